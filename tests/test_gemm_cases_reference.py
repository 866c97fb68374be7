"""CPU: keeps tests/gemm_cases.py honest in both directions at small shapes: the fp32 emulation in the kernels' order and the
stock fp32 torch.nn.functional.linear lie inside every bound (ratios printed) and equal the rounded float64 reference bit for
bit on the exact kinds, every named mutation lands outside a bound and breaks the exact equality, and the library's host
entry gf_gemm_plan agrees with the restated launch arithmetic on every table entry -- so that a retuned grid fails here
instead of silently turning every GPU case into one tile per workgroup."""
import ctypes

import pytest
import torch

import gemm_cases as G

F32, BF16 = torch.float32, torch.bfloat16
dtypes = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])

# (M, N, K0, K1, nres, rot_n): small, every epilogue combination the kernels have
SMALL = [(96, 64, 32, 0, 0, 0), (96, 64, 64, 0, 1, 0), (70, 96, 32, 32, 2, 0), (96, 128, 64, 64, 1, 64), (65, 128, 128, 0, 1, 128),
         (128, 128, 256, 0, 0, 128), (96, 96, 16, 16, 1, 64), (128, 256, 256, 256, 2, 0)]
SMALL_BG = [(2, 5, 7, 29, "kc", "kc"), (1, 33, 17, 64, "kc", "rc"), (3, 17, 40, 70, "rc", "kc"), (2, 40, 9, 33, "rc", "rc"),
            (1, 9, 12, 65, "nu", "mis"), (2, 130, 3, 5, "mis", "nu")]


def _cases(dtype, kinds=G.KINDS):
    for shape in SMALL:
        for kind in kinds:
            yield G.gemm_case(kind, *shape, dtype)


def _bg_cases(dtype, kinds=("rand", "exact")):
    for shape in SMALL_BG:
        for kind in kinds:
            yield G.bgemm_case(kind, *shape, dtype)


@dtypes
def test_emulation_and_stock_inside_and_exact(dtype):
    worst = {"emulation": 0.0, "stock": 0.0, "bgemm": 0.0}
    for case in _cases(dtype):
        ref = G.gemm_ref(case)
        for name, stock in (("emulation", False), ("stock", True)):
            y = G.emulate_gemm(case, stock)
            worst[name] = max(worst[name], G.ratio(y, ref["y"], ref["y_bound"]))
            if case["kind"] in G.EXACT_KINDS:
                assert torch.equal(y.double(), ref["rounded"]), (name, case["kind"], case["M"], case["N"], case["K0"])
    for case in _bg_cases(dtype):
        ref = G.bgemm_ref(case)
        c = G.emulate_bgemm(case)
        worst["bgemm"] = max(worst["bgemm"], G.ratio(c, ref["c"], ref["c_bound"]))
        if case["kind"] == "exact":
            assert torch.equal(c.double(), ref["rounded"]), (case["M"], case["N"], case["K"])
    print(f"gemm {str(dtype)[6:]}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_reference_is_linear_plus_rotate_half():
    """The restated reference against torch's own float64 linear and the rotation written with complex numbers."""
    case = G.gemm_case("rand", 96, 128, 64, 64, 1, 64, F32)
    ref = G.gemm_ref(case)["y"]
    s = torch.nn.functional.linear(torch.cat((case["x0"], case["x1"]), 1).double(), case["w"].double(), case["bias"].double())
    s = s + case["res"].double()
    z = torch.view_as_complex(s[:, :64].reshape(96, 32, 2).contiguous())
    rot = torch.view_as_real(z * torch.view_as_complex(case["cs"].double().reshape(96, 32, 2).contiguous())).reshape(96, 64)
    torch.testing.assert_close(ref, torch.cat((rot, s[:, 64:]), 1), rtol=1e-13, atol=1e-13)


def _mutations(cases_of, ref_of, mutations, out):
    """Worst ratio of each mutation on rand / cancel, mismatch count on the exact kinds; every mutation must show in both."""
    hit = {m: 0.0 for m in mutations}
    wrong = {m: 0 for m in mutations}
    for dtype in (F32, BF16):
        for case in cases_of(dtype):
            ref = ref_of(case)
            for m, applies in mutations.items():
                if not applies(case):
                    continue
                mut = ref_of(case, m)
                if case["kind"] in G.EXACT_KINDS:
                    wrong[m] += int((mut["rounded"] != ref["rounded"]).sum())
                else:
                    hit[m] = max(hit[m], G.ratio(mut[out], ref[out], ref[out + "_bound"]))
    print("; ".join(f"{m} {hit[m]:.3g} bounds, {wrong[m]} exact mismatches" for m in mutations))
    for m in mutations:
        assert hit[m] > G.DETECT, f"mutation {m} stays inside the bound ({hit[m]:.3g})"
        assert wrong[m] > 0, f"mutation {m} leaves every exact case bit-equal"


def test_gemm_mutations_outside():
    """y is the one asserted output of the GEMM entries: every mutation moves it."""
    _mutations(_cases, G.gemm_ref, G.GEMM_MUTATIONS, "y")


def test_bgemm_mutations_outside():
    _mutations(_bg_cases, G.bgemm_ref, G.BGEMM_MUTATIONS, "c")


# ================================================================================================ the launch arithmetic
def _plan(L, M, N, K0, K1, nres, rot_n, dtype=G.GF_BF16):
    out = (ctypes.c_int64 * 11)()
    code = L.gf_gemm_plan(M, N, K0, K1, int(nres >= 1), int(nres == 2), int(rot_n > 0), rot_n, dtype, out)
    return code, list(out)


def _split(K, two):
    return (K // 2, K // 2) if two else (K, 0)


def test_gemm_plan_matches_the_restated_tile_arithmetic():
    """Every gemm_st instance is exercised at a smallest launch, at T = 1 everywhere and at the ragged {2,1}, {3,2}, {4,3}."""
    from glue_factory_amd import lib
    L = lib.load()
    assert len(set(G.ST_INSTANCES)) == 14
    for K, two, nres, rot in G.ST_INSTANCES:
        K0, K1 = _split(K, two)
        seen = []
        for M, want in G.ST_M[K]:
            rot_n = G.ST_N if rot else 0
            code, out = _plan(L, M, G.ST_N, K0, K1, nres, rot_n)
            tr, gx, gy, tmin, tmax = G.st_plan(M, G.ST_N, K)
            assert code == 1 and out[:6] == [1, gx, gy, tr, tmin, tmax] and out[6:] == [0] * 5, \
                f"gf_gemm_plan({M}, {G.ST_N}, K = {K}) = {code}, {out}: the tables of gemm_cases.py restate {(gx, gy, tr, tmin, tmax)}"
            assert {tmin, tmax} == want, f"M = {M}, K = {K}: tile counts {{{tmax},{tmin}}}, the table promises {want}"
            assert tr == (64 if K == 256 else 32) and gy == 8 and gx == min(32, M // tr)
            assert G.st_serves(M, G.ST_N, K0, K1, nres, rot_n, BF16)
            seen.append((tmax, tmin))
            # one more row: the register-resident kernel (gf_gemm), nothing at all for two residuals (gf_gemm_res2)
            code, out = _plan(L, M + 1, G.ST_N, K0, K1, nres, rot_n)
            assert code == (G.GF_ERR_UNSUPPORTED if nres == 2 else 0)
            if nres < 2:
                rows = G.ws_rows(K, BF16)
                assert out[:6] == [1, -(-(M + 1) // rows), 1, rows, 1, 1]
        assert seen[0] == (1, 1) and G.ST_M[K][0][0] == 64, "the smallest launch"
        assert seen[1:] == [(1, 1), (2, 1), (3, 2), (4, 3)], (K, two, nres, rot, seen)
        assert G.ST_RAGGED_M[K] == G.ST_M[K][2][0]
        for M, N, want in G.ST_NARROW[K]:
            code, out = _plan(L, M, N, K0, K1, nres, N - N % 256 if rot else 0)
            tr, gx, gy, tmin, tmax = G.st_plan(M, N, K)
            assert code == 1 and out[:6] == [1, gx, gy, tr, tmin, tmax] and {tmin, tmax} == want, (M, N, K, out)
    for K in (256, 512):                      # rotary with rot_n < N: a second, plain launch over one channel group
        for N, rot_n in G.ST_ROT_N:
            M = G.ST_RAGGED_M[K]
            code, out = _plan(L, M, N, K, 0, 0, rot_n)
            first = [*G.st_plan(M, rot_n, K)]
            first = [first[1], first[2], first[0], first[3], first[4]]
            if N == rot_n:
                assert code == 1 and out == [1] + first + [0] * 5
            else:
                tr, gx, gy, tmin, tmax = G.st_plan(M, N - rot_n, K)
                assert code == 1 and out == [2] + first + [gx, gy, tr, tmin, tmax] and gy == 1


def test_gemm_plan_register_resident_blocks_and_rejections():
    from glue_factory_amd import lib
    L = lib.load()
    for dtype, code_dt in ((BF16, G.GF_BF16), (F32, G.GF_F32)):
        for K in G.WS_K[dtype]:
            for M in G.WS_M:
                code, out = _plan(L, M, 96, K, 0, 1, 64, code_dt)
                rows = G.ws_rows(K, dtype)
                assert code == 0 and out[:6] == [1, -(-M // rows), 1, rows, 1, 1], (K, M, out)
        for K0 in G.WS_TWO_K0[dtype]:
            assert _plan(L, 33, 32, K0, K0, 0, 0, code_dt)[0] == 0
    assert _plan(L, 64, 256, 512, 0, 0, 0, G.GF_F32)[0] == G.GF_ERR_UNSUPPORTED            # fp32 stops at K = 256
    assert _plan(L, 64, 256, 48, 0, 0, 0)[0] == G.GF_ERR_UNSUPPORTED                       # no instance for K = 48
    assert _plan(L, 64, 40, 64, 0, 0, 0)[0] == G.GF_ERR_UNSUPPORTED                        # N % 32
    assert _plan(L, 64, 64, 64, 32, 0, 0)[0] == G.GF_ERR_UNSUPPORTED                       # K1 != K0
    assert _plan(L, 64, 128, 64, 0, 0, 32)[0] == G.GF_ERR_SHAPE                            # rot_n % 64
    assert _plan(L, 64, 128, 64, 0, 0, 192)[0] == G.GF_ERR_SHAPE                           # rot_n > N
    assert _plan(L, 64, 128, 64, 0, 0, 0, 7)[0] == G.GF_ERR_DTYPE
    assert _plan(L, 0, 128, 64, 0, 0, 0)[0] == G.GF_ERR_SHAPE
    assert _plan(L, 64, 256, 256, 0, 2, 0, G.GF_F32)[0] == G.GF_ERR_UNSUPPORTED            # gf_gemm_res2 is bf16 only
    assert _plan(L, 64, 128, 256, 0, 2, 0)[0] == G.GF_ERR_UNSUPPORTED                      # ... and the streamed shapes only
    assert _plan(L, 64, 256, 256, 0, 2, 0)[0] == 1
    # rotary with a residual, with two sources or at rot_n % 256 != 0 is the register-resident kernel's
    assert _plan(L, 64, 256, 256, 0, 1, 256)[0] == 0 and _plan(L, 64, 256, 128, 128, 0, 256)[0] == 0
    assert _plan(L, 64, 256, 256, 0, 0, 64)[0] == 0 and _plan(L, 64, 256, 256, 0, 0, 256)[0] == 1
