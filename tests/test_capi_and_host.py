"""CPU-only checks: the C-ABI library builds/loads and exports every symbol declared in
include/gf_amd.h; config object, plugin registry and BaseModel semantics; the product path
fails loudly without a GPU (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from glue_factory_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    declared = _declared_symbols()
    assert len(declared) >= 12
    for name in declared:
        assert hasattr(so, name), f"{name} declared in gf_amd.h but not exported"
    assert set(declared) == set(lib.SIGNATURES), set(declared) ^ set(lib.SIGNATURES)
    assert lib.load().gf_abi_version() == lib.ABI_VERSION


def test_conf_semantics():
    from glue_factory_amd.conf import Conf, ConfError
    base = Conf.create({"a": 1, "loss": {"gamma": 1.0, "fn": "nll"}, "layers": ["self", "cross"]})
    c = Conf.merge(base, {"a": 2, "loss": {"gamma": 0.5}})
    assert c.a == 2 and c.loss.gamma == 0.5 and c.loss.fn == "nll" and c["layers"] == ["self", "cross"]
    assert base.a == 1  # merge does not alias
    c.set_struct(True)
    with pytest.raises(ConfError):
        c.unknown
    with pytest.raises(ConfError):
        c["new"] = 1
    with pytest.raises(ConfError):
        Conf.merge(c, {"nope": 1})
    c.set_readonly(True)
    with pytest.raises(ConfError):
        c.a = 5
    assert c.to_container() == {"a": 2, "loss": {"gamma": 0.5, "fn": "nll"}, "layers": ["self", "cross"]}
    d = Conf.from_dotlist(["model.matcher.n_layers=4", "train.lr=1e-4", "x=true"])
    assert d.model.matcher.n_layers == 4 and d.x is True


def test_registry_and_base_model():
    from glue_factory_amd.base_model import BaseModel, get_model

    LG = get_model("glue_factory_amd.matchers.lightglue")
    assert LG.__name__ == "LightGlue"
    assert get_model("matchers.lightglue") is LG and get_model("lightglue") is LG
    with pytest.raises(RuntimeError):
        get_model("does.not.exist")

    class Child(BaseModel):
        default_conf = {"k": 3, "nested": {"x": 1}}
        required_data_keys = ["view0"]

        def _init(self, conf):
            self.lin = torch.nn.Linear(2, 2)
            self.bn = torch.nn.BatchNorm1d(2)

        def _forward(self, data):
            return {"y": data["view0"]}

        def loss(self, pred, data):
            raise NotImplementedError

    m = Child({"nested": {"x": 5}, "trainable": False, "freeze_batch_normalization": True, "extra": 1})
    assert m.conf.k == 3 and m.conf.nested.x == 5 and m.conf.name is None and m.conf.extra == 1
    assert all(not p.requires_grad for p in m.parameters())
    m.train()
    assert m.training and not m.bn.training
    with pytest.raises(AssertionError):
        m({})
    assert m({"view0": 1}) == {"y": 1}
    assert not m.is_initialized()
    m.load_state_dict(m.state_dict())
    assert m.is_initialized()


def test_lightglue_conf_state_dict_and_no_cpu_fallback():
    from glue_factory_amd.matchers.lightglue import LightGlue
    from oracle import lightglue_oracle as lgo
    m = LightGlue({"n_layers": 2, "checkpointed": True, "flash": False})
    ref = lgo.init_params(2, 256, 4, seed=0)
    sd = m.state_dict()
    assert set(sd) == set(ref) and all(sd[k].shape == ref[k].shape for k in ref)
    torch.testing.assert_close(sd["confidence_thresholds"], ref["confidence_thresholds"])
    data = {"keypoints0": torch.rand(1, 8, 2), "keypoints1": torch.rand(1, 8, 2),
            "descriptors0": torch.rand(1, 8, 256), "descriptors1": torch.rand(1, 8, 256)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(data)
    assert LightGlue({"descriptor_dim": 128, "num_heads": 4, "n_layers": 1}).posenc.Wr.weight.shape == (16, 2)   # head_dim 32: generic kernels
    with pytest.raises(NotImplementedError):
        LightGlue({"descriptor_dim": 192, "num_heads": 4})                                                       # head_dim 48: no kernel


def test_fixed_length_positive_list_equals_nonzero():
    """LightGlue._gt_sparse: the fixed-length list built from gt_assignment_col0 carries the same positives
    and counts as nonzero() on the dense matrix (host logic, CPU)."""
    import torch
    from glue_factory_amd.matchers.lightglue import LightGlue
    from glue_factory_amd.synthetic import make_pairs
    data = make_pairs(3, 50, 60, dim=8, size=(640, 480), seed=4)
    dense = LightGlue._gt_sparse(data)
    fixed = LightGlue._gt_sparse(data, fixed=True)
    assert fixed["pos"][2].shape[0] == 3 * 50
    keep = fixed["pos"][2] >= 0
    got = torch.stack([t[keep] for t in fixed["pos"]], 1)
    ref = torch.stack(dense["pos"], 1)
    assert torch.equal(got, ref)                       # same (b, i, j) triples in the same (sorted) order
    for k in ("num_pos", "n0", "n1", "neg0", "neg1"):
        assert torch.equal(fixed[k], dense[k]), k
    data.pop("gt_assignment_col0")
    again = LightGlue._gt_sparse(data, fixed=True)     # producer without the key: dense path
    assert torch.equal(torch.stack(again["pos"], 1), ref)


def test_precast_cache_follows_parameter_versions():
    import torch
    from glue_factory_amd import ops
    if not torch.cuda.is_available():
        # CPU tensors are never cached (the product path is HIP-only): _lp is a plain cast
        w = torch.nn.Parameter(torch.randn(4, 4))
        ops.precast([w], torch.bfloat16, key="t")
        assert ops._lp(w, torch.bfloat16).dtype == torch.bfloat16
        assert id(w) not in ops._LP_CACHE


def test_ops_package_surface_and_global_state(monkeypatch):
    """glue_factory_amd.ops (`pkg` here, so that this test adds nothing to its own scan) is a package of one sub-module per
    kernel family: (a) every attribute of it that the repository names resolves on the package, (b) each mutable global
    container is the SAME object on the package and in its home module, (c) the rebindable switches are attributes of the
    package alone and their consumers read them there at call time."""
    import glob
    import types
    from glue_factory_amd import lib, ops as pkg
    assert os.path.basename(pkg.__file__) == "__init__.py"

    # (a) the names used by the modules that import `ops` from this package
    files = [os.path.join(ROOT, "bench.py")] + glob.glob(os.path.join(ROOT, "tests", "*.py"))
    files += glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "glue-factory_amd", "**", "*.py"), recursive=True)
    imports_ops = re.compile(r"^\s*from\s+(glue_factory_amd|\.\.?)\s+import\s+.*\bops\b", re.M)
    used = set()
    for path in files:
        text = open(path).read()
        if imports_ops.search(text):
            used |= set(re.findall(r"\b_?ops\.([A-Za-z_]\w*)", text))
    missing = sorted(n for n in used if not hasattr(pkg, n))
    assert not missing, missing
    assert len(used) >= 59, len(used)          # distinct names this scan found while the package was still one module

    # (b) one home per container, re-exported by identity
    homes = {"_LP_CACHE": pkg._params, "_LP_PTR": pkg._params, "_LP_T": pkg._params, "_LP_FLAT": pkg._params,
             "LIBRARY_GEMMS": pkg._linear, "_SPARSE_SUMS": pkg._nll, "COLLECTIVES": pkg._batchnorm}
    subs = [m for n, m in vars(pkg).items() if isinstance(m, types.ModuleType) and m.__name__ == pkg.__name__ + "." + n]
    assert len(subs) == 9
    for name, home in homes.items():
        assert getattr(pkg, name) is getattr(home, name), name
        assert [m for m in subs if hasattr(m, name)] == [home], name
    cache = pkg._LP_CACHE
    pkg.invalidate_precast()                   # ... and mutated in place, never rebound
    assert pkg._LP_CACHE is cache is pkg._params._LP_CACHE

    # (c) the switches: no copy in any sub-module
    for name in ("XBWD_ENABLED", "FOLD_ENABLED", "REPLAY_GATE", "FORCE_SYNC_BN"):
        assert hasattr(pkg, name) and not [m.__name__ for m in subs if hasattr(m, name)], name

    class Consulted(Exception):
        pass

    class Sentinel:
        def __bool__(self):
            raise Consulted

    def launched(*a, **k):
        raise AssertionError("a consumer ignored the package switch and went on to the library")
    monkeypatch.setattr(lib, "load", launched)
    # _CrossAttentionStacked.backward takes the truth value of the package's XBWD_ENABLED before it picks a kernel
    p = torch.zeros(2, 64, 2, 4, 64, dtype=torch.bfloat16)
    ctx = types.SimpleNamespace(saved_tensors=(p, torch.zeros(2, 64, 4, 64, dtype=torch.bfloat16), torch.zeros(2, 4, 64)),
                                scale=pkg.LN2)
    monkeypatch.setattr(pkg, "XBWD_ENABLED", Sentinel())
    with pytest.raises(Consulted):
        pkg._attention._CrossAttentionStacked.backward(ctx, torch.zeros(2, 64, 4, 64, dtype=torch.bfloat16))
    # folded_linear: a prepared fold is ignored while the package's FOLD_ENABLED is off, and consulted while it is on
    monkeypatch.setitem(pkg._LP_FLAT, ("t_fold", torch.bfloat16), {"derived": {"f": {"fold": (1, 1, 1, 1, 0)}}})
    monkeypatch.setattr(pkg, "FOLD_ENABLED", False)
    assert pkg.folded_linear("t_fold", torch.bfloat16, "f", None, None, None, None) is None
    monkeypatch.setattr(pkg, "FOLD_ENABLED", Sentinel())
    with pytest.raises(Consulted):
        pkg.folded_linear("t_fold", torch.bfloat16, "f", None, None, None, None)


def test_sinkhorn_resident_plan_is_consistent():
    """gf_sinkhorn_plan (host-only): the distribution of the chip-resident Sinkhorn sweeps (csrc/sinkhorn_resident.hip) over a
    256-CU device -- every pair gets whole workgroups, every row a wave, the rows of a wave fit its registers + LDS share, the
    column phase covers every float4 column, the LDS request stays inside the CU -- for the benchmarked geometry and around it."""
    import ctypes
    from glue_factory_amd import lib
    L = lib.load()
    out = (ctypes.c_int64 * 8)()
    seen = 0
    for B in (1, 4, 5, 7, 8, 9, 16, 20, 32, 33, 64):
        for M in (255, 1000, 2048):
            for N in (256, 512, 1024, 1280, 2048):
                for bwd in (0, 1):
                    ok = L.gf_sinkhorn_plan(B, M, N, 256, bwd, 1, out)
                    assert ok in (0, 1)
                    if B < 5:
                        assert ok == 0                                    # few pairs stay on the streaming kernels
                    if not ok:
                        continue
                    seen += 1
                    bc, wpp, nw, base, extra, cs, nsm, lds = (int(v) for v in out)
                    R, nvec = M + 1, N // 4 + 1
                    assert 5 <= bc <= min(B, 16) and wpp * bc <= 256 and nw == 4 * wpp and nsm == N // 256
                    assert base * nw + extra == R and 0 <= extra < nw               # every row has exactly one wave
                    assert base + (1 if extra else 0) <= 64                          # per-row scalars live one per lane
                    assert cs * wpp >= nvec and cs <= 32                             # the column phase covers every column
                    lds_rows = sum(max(0, base + (1 if w < extra else 0) - 12) for w in range(4))
                    assert lds == ((2 if bwd else 1) * (N // 4) + 256) * 16 + 32 + lds_rows * (N // 4) * 16
                    assert lds <= 160 * 1024 - 512
                    # launches cover the batch with balanced chunks
                    nch = -(-B // bc)
                    assert (nch - 1) * bc < B <= nch * bc
    assert seen > 50
    assert L.gf_sinkhorn_plan(32, 2048, 2048, 256, 0, 1, out) == 1 and tuple(out)[:5] == (8, 32, 128, 16, 1)
    assert L.gf_sinkhorn_plan(32, 2048, 2050, 256, 0, 1, out) == 0                      # N % 256 != 0: streaming
    assert L.gf_sinkhorn_plan(32, 2048, 2304, 256, 0, 1, out) == 0                      # N / 256 > 8


# (M, N) across the tier boundaries of gf_sinkhorn_fwd / _bwd: ragged N (streaming only), N = 256 .. 2304 in steps the resident
# layout accepts (N / 256 <= 8), N + 1 = 2304 (the last streaming width), N + 1 > 2304 (generic LDS kernels), M != N both ways,
# and a width whose rows no longer fit the LDS (unsupported)
_SK_SHAPES = ((255, 250), (256, 256), (1000, 512), (300, 1024), (1500, 1280), (2047, 2048), (2048, 2048), (2048, 2050),
              (2048, 2303), (2304, 2304), (2400, 2400), (100, 3000), (3000, 300), (64, 9000))
_SK_BATCHES = (1, 4, 5, 8, 9, 17, 32)
# 64 / 256 / 304 CUs: parts that exist.  512: no such part, but the only way to a plan with more partial rows (4 waves per
# workgroup x workgroups) than the workspace reserves (4 x 320) -- the condition that sends such a call to the streaming kernels
_SK_NCU = (64, 256, 304, 512)


def _sinkhorn_host_record(L):
    out = (ctypes.c_int64 * 8)()
    ws, plan = {}, {}
    for B in _SK_BATCHES:
        for M, N in _SK_SHAPES:
            for iters in (0, 1, 100):
                ws[f"{B},{M},{N},{iters}"] = int(L.gf_sinkhorn_ws_bytes(B, M, N, iters))
            for ncu in _SK_NCU:
                for bwd in (0, 1):
                    for mode in (0, 1, 2):
                        ok = int(L.gf_sinkhorn_plan(B, M, N, ncu, bwd, mode, out))
                        plan[f"{B},{M},{N},{ncu},{bwd},{mode}"] = [ok] + ([int(v) for v in out] if ok == 1 else [])
    return {"ws_bytes": ws, "plan": plan}


def test_sinkhorn_host_arithmetic_matches_recorded():
    """gf_sinkhorn_ws_bytes and gf_sinkhorn_plan (both host-only) against tests/golden/sinkhorn_host.json, this library's own
    output recorded before the Sinkhorn translation unit was split: workspace sizes, which calls take the chip-resident
    sweeps and with which distribution, over B x (M, N) x iterations x direction x schedule mode x CU count.  Whoever
    changes the workspace layout or the tier selection on purpose re-records the file (json.dump of _sinkhorn_host_record)."""
    import json
    from glue_factory_amd import lib
    got = _sinkhorn_host_record(lib.load())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "sinkhorn_host.json")))
    assert got["ws_bytes"] == want["ws_bytes"]
    assert got["plan"] == want["plan"]
    assert sum(v[0] == 1 for v in want["plan"].values()) > 100
    # the fixture holds calls that the partial-row reservation alone keeps off the resident path (more CUs only shrink
    # every other requirement of the plan)
    def at256(key):
        f = key.split(",")
        return ",".join(f[:3] + ["256"] + f[4:])
    assert any(k.split(",")[3] == "512" and v[0] == 0 and want["plan"][at256(k)][0] == 1 for k, v in want["plan"].items())


# M: the train step's token count, every M of test_linear_dw / test_linear_cat_weight_gradient_in_one_launch / the ragged-slice
# test, and the edges of plan()'s 256-row minimum and 64-row rounding.  (Nout, K): the step's five shapes, every shape those tests
# reach (the two-source ones whole and per source), 64 tiles (1024 x 1024: one per slot of an XCD) and 80 (more than its slots)
_DW_M = (1, 64, 255, 256, 257, 300, 777, 1000, 2049, 4096, 4133, 5000, 131072)
_DW_SHAPES = ((8, 8), (136, 72), (264, 136), (128, 128), (128, 256), (256, 128), (256, 256), (256, 384), (256, 512), (512, 256),
              (512, 512), (768, 256), (1024, 1024), (1280, 1024))
_DW_INVALID = ((0, 256, 256), (-1, 256, 256), (1000, 0, 256), (1000, 256, 0), (1000, -8, 256), (1000, 256, -128), (0, 0, 0))


def _linear_dw_host_record(L):
    return {f"{m},{n},{k}": int(L.gf_linear_dw_ws_bytes(m, n, k))
            for m, n, k in [(m, n, k) for m in _DW_M for n, k in _DW_SHAPES] + list(_DW_INVALID)}


def test_linear_dw_workspace_matches_recorded():
    """gf_linear_dw_ws_bytes (host-only: the slice plan of csrc/linear_dw.hip) against tests/golden/linear_dw_host.json, this
    library's own output recorded before the weight-gradient translation unit got its one launch path.  Whoever changes the
    slice plan or the workspace layout on purpose re-records the file (json.dump of _linear_dw_host_record)."""
    import json
    from glue_factory_amd import lib
    got = _linear_dw_host_record(lib.load())
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "linear_dw_host.json")))
    assert got == want
    assert all(want[f"{m},{n},{k}"] == -2 for m, n, k in _DW_INVALID)                     # GF_ERR_SHAPE
    assert all(v > 256 for key, v in want.items() if tuple(int(f) for f in key.split(",")) not in _DW_INVALID)
    # the fixture tells the plan's branches apart: one slice (M below the 256-row minimum), a ragged last slice, the 64-row
    # rounding (2049 rows for 8 slices: 257 -> 320 rows, 7 slices), slices per XCD clamped to 1 above 64 tiles, and the
    # step's 512 slots / 4 tiles
    slices = lambda m, n, k: (want[f"{m},{n},{k}"] - 256) // (4 * (n * k + n))
    assert slices(255, 256, 256) == 1 and slices(257, 256, 256) == 2 and slices(2049, 1024, 1024) == 7
    assert slices(131072, 1024, 1024) == 8 == slices(131072, 1280, 1024) and slices(131072, 256, 256) == 128


def _unknown_dtype_calls(L, lib):
    """One call per dtype-taking entry point: valid small shapes, null data pointers, dtype code 7."""
    N, DT = None, 7
    s = lib.strides(4096, 64, 64)               # [B, 64 tokens, 1 head, 64] in elements: batch, token, head
    g = lib.strides(64, 8, 1)                   # [batch, 8, 8] row-major
    plan_out = lib.strides(*([0] * 11))         # gf_gemm_plan's result array (it rejects a null one first)
    return {
        "gf_attn_fwd": lambda: L.gf_attn_fwd(N, N, N, N, N, 1, 1, 64, 64, 64, s, s, s, s, 1.0, DT, N),
        "gf_attn_fwd_ex": lambda: L.gf_attn_fwd_ex(N, N, N, N, N, 1, 1, 64, 64, 64, s, s, s, s, 1.0, DT, 0, N, N),
        "gf_attn_bwd": lambda: L.gf_attn_bwd(N, N, N, N, N, N, N, N, N, N, 1, 1, 64, 64, 64, s, s, s, s, s, s, s, s, 1.0, DT, N),
        "gf_attn_bwd_acc": lambda: L.gf_attn_bwd_acc(N, N, N, N, N, N, N, N, N, N, 1, 1, 64, 64, 64, s, s, s, s, s, s, s, s, 1.0,
                                                     DT, 0, N),
        "gf_rows_lse": lambda: L.gf_rows_lse(N, N, N, N, 1, 8, 8, 64, DT, N),
        "gf_rows_argmax": lambda: L.gf_rows_argmax(N, N, N, 1.0, N, N, 1, 8, 8, 64, DT, N),
        "gf_assign_write": lambda: L.gf_assign_write(N, N, N, N, N, N, 1.0, 0.0, N, N, 1, 8, 8, 64, DT, N),
        "gf_dual_softmax_bwd": lambda: L.gf_dual_softmax_bwd(N, N, N, N, N, N, N, 8, 1.0, N, 1, 8, 8, 64, DT, N),
        "gf_line_gather": lambda: L.gf_line_gather(N, N, N, N, 1, 8, 8, 64, DT, N),
        "gf_line_segsum": lambda: L.gf_line_segsum(N, 64, N, 0, N, N, N, N, 1, 8, 8, 64, 0, DT, N),
        "gf_line_expand": lambda: L.gf_line_expand(N, N, N, N, 1, 8, 8, 64, 0, DT, N),
        "gf_rows_gather": lambda: L.gf_rows_gather(N, N, N, 1, 8, 8, 64, DT, N),
        "gf_multi_cast_transpose": lambda: L.gf_multi_cast_transpose(N, 1, 1, DT, N),
        "gf_bgemm": lambda: L.gf_bgemm(N, N, N, 1, 8, 8, 8, g, g, g, 1.0, DT, N),
        "gf_gemm": lambda: L.gf_gemm(N, N, N, N, N, N, N, 0, 64, 32, 32, 0, 32, 0, 32, 0, 32, DT, N),
        "gf_gemm_plan": lambda: L.gf_gemm_plan(64, 32, 32, 0, 0, 0, 0, 0, DT, plan_out),
        "gf_linear_dw": lambda: L.gf_linear_dw(N, N, N, N, N, 64, 8, 8, DT, N),
        "gf_bn_stats": lambda: L.gf_bn_stats(N, N, 8, 8, DT, N),
        "gf_bn_act_fwd": lambda: L.gf_bn_act_fwd(N, N, N, N, N, N, 8, 8, 0, DT, N),
        "gf_bn_bwd_stats": lambda: L.gf_bn_bwd_stats(N, N, N, N, N, N, N, 8, 8, 0, DT, N),
        "gf_bn_bwd_dx": lambda: L.gf_bn_bwd_dx(N, N, N, N, N, N, N, N, N, 8, 8, 0, DT, N),
        "gf_wf_descriptors": lambda: L.gf_wf_descriptors(N, N, N, N, N, 1, 8, 0, 4, 4, 64, 8, DT, N),
        "gf_bias_act_bn_nhwc": lambda: L.gf_bias_act_bn_nhwc(N, N, N, N, N, 1, 8, 8, 64, 0, 0, DT, N),
        "gf_conv1_bias_act_bn": lambda: L.gf_conv1_bias_act_bn(N, N, N, N, N, N, 1, 8, 8, 64, 0, DT, N),
        "gf_conv3x3_c64": lambda: L.gf_conv3x3_c64(N, N, N, N, N, N, 1, 8, 8, 0, 0, DT, N),
        "gf_conv3x3_c64_ld": lambda: L.gf_conv3x3_c64_ld(N, N, N, N, N, N, 64, 1, 8, 8, 0, 0, DT, N),
        "gf_detector_scores": lambda: L.gf_detector_scores(N, N, N, N, N, 1, 4, 4, 0, DT, N),
        "gf_sample_descriptors": lambda: L.gf_sample_descriptors(N, N, N, 1, 8, 4, 4, 64, 8, DT, N),
        "gf_rowdot_fwd": lambda: L.gf_rowdot_fwd(N, N, 0.0, N, N, 8, 8, DT, N),
        "gf_rowdot_bwd": lambda: L.gf_rowdot_bwd(N, N, N, N, N, N, 8, 8, DT, N),
        "gf_rowdot2_fwd": lambda: L.gf_rowdot2_fwd(N, N, N, N, N, N, N, 8, 8, DT, N),
        "gf_rowdot2_bwd": lambda: L.gf_rowdot2_bwd(N, N, N, N, N, N, N, 8, 8, DT, N),
        "gf_lg_loss_fwd": lambda: L.gf_lg_loss_fwd(N, N, N, N, N, N, N, N, N, 0, N, N, N, N, N, N, N, N, N, N, N, N, N,
                                                   1, 8, 8, 64, DT, N),
        "gf_lg_loss_bwd_rows": lambda: L.gf_lg_loss_bwd_rows(N, N, N, N, N, 1, N, N, N, 1, 8, 8, 64, DT, N),   # P = 0 returns 0 first
        "gf_rotary_qk": lambda: L.gf_rotary_qk(N, N, 1, 8, 4, 64, 0, DT, N),
        "gf_rotary_qk_bwd": lambda: L.gf_rotary_qk_bwd(N, N, N, N, N, 1, 8, 4, 64, DT, N),
        "gf_ln_gelu_fwd": lambda: L.gf_ln_gelu_fwd(N, N, N, N, N, N, 8, 256, 1e-5, DT, N),
        "gf_ln_gelu_bwd": lambda: L.gf_ln_gelu_bwd(N, N, N, N, N, N, N, N, N, 8, 256, DT, N),
    }


def test_unknown_dtype_code_is_rejected_before_any_launch():
    """Every entry point that takes a dtype answers GF_ERR_DTYPE (-4) for a code that is neither fp32 (0) nor bf16 (1), with
    otherwise valid arguments and before it touches a pointer or the device (csrc/gf_launch.h: gf_by_dtype).
    Not in the table, because null pointers cannot pass their earlier checks: gf_rows_lse_argmax, gf_rows_top2 and gf_hv_warp
    (GF_ERR_SHAPE for a null output / input) and gf_linear_dw2 (GF_ERR_UNSUPPORTED for a null source).  The bf16-only entry
    points answer GF_ERR_UNSUPPORTED (-1) for every other code, fp32 included, in one test with the head_dim: pinned below."""
    from glue_factory_amd import lib
    L = lib.load()
    calls = _unknown_dtype_calls(L, lib)
    got = {name: call() for name, call in calls.items()}
    assert got == {name: -4 for name in calls}
    # every dtype-taking declaration is either in the table or named above
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gf_amd.h")).read(), flags=re.S)
    takes_dtype = {m.group(1) for m in re.finditer(r"\b(gf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text) if "dtype" in m.group(2)}
    bf16_only = {"gf_attn_cross_bwd", "gf_head_bwd", "gf_gemm_res2"}
    left_out = {"gf_rows_lse_argmax", "gf_rows_top2", "gf_hv_warp", "gf_linear_dw2"}
    assert takes_dtype == set(calls) | bf16_only | left_out
    N, s = None, lib.strides(4096, 64, 64)
    assert L.gf_attn_cross_bwd(N, N, N, N, N, N, N, N, 2, 1, 1, 64, 64, s, s, s, s, s, s, 1.0, 7, N) == -1
    assert L.gf_head_bwd(N, N, N, N, N, N, N, N, 1, 8, 8, 256, 7, N) == -1
    assert L.gf_gemm_res2(N, N, N, N, N, N, N, 64, 256, 256, 0, 256, 0, 256, 256, 256, 256, 7, N) == -1
