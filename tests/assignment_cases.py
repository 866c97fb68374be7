"""Shared by tests/test_assignment_cases_reference.py (CPU) and tests/test_gpu_assignment.py: seeded inputs, float64
references, an fp32 rounding model and the derived error bounds of the assignment head kernels (csrc/assignment.hip;
contract in include/gf_amd.h).  No GPU code and no library code here.

Geometry.  Every kernel keeps 128 rows of an OWNER matrix in registers and streams the other matrix in 64-row tiles;
gf_assign_write and gf_dual_softmax_bwd also divide the streamed rows among four workgroups (split_ranges).  A case is
therefore stated as own [B,No,D], oth [B,Ns,D] and S[b,o,s] = own_o . oth_s, and is used in both roles: the lse / arg-max
entries get (a, b) = (own, oth) and reduce over s; assign_write / dual_softmax_bwd get (a, b) = (oth, own), so their output
is [B, Ns(+1), No(+1)].  Descriptors are taken as stored: a bf16 tensor is upcast to float64 and never rounded again.

Next to every reference value stands `T`, the sum of the absolute values of its elementary addends (the D products of
S, every bias and normaliser separately, the three terms of dS): what an fp32 evaluation's error is proportional to.

Bounds (derived, not tuned; U = 2^-24, the fp32 rounding unit):
  value       |x - ref| <= C_ACC T + FLOOR, C_ACC = 1e-5, FLOOR = 1e-6.  Worst-case sequential fp32 accumulation of D = 256
              products is D U T = 1.5e-5 T, reached only when every partial sum is as large as T and every rounding falls
              the same way; the rounding model (sequential fp32) stays below 1e-5 T in every case here, which the CPU test
              asserts.  bf16 inputs add nothing: the reference upcasts the stored values, and a product of two bf16 values
              is exact in fp32.
  lse         the same with T = max_j T_ij + |lse_i|: the exp2 / log2 error acts on the shifted scores (<= 0, each a few U
              of T_ij off), and the final (m + log2 sum) ln 2 rounds relative to |lse|.
  dS          sum over the two softmax terms t of |t| (3 U (|S| + |n|) + 8 U + C_ACC T_S + FLOOR): the exp2 argument
              (S - n) log2 e is formed with three roundings of quantities of size (|S| + |n|) log2 e, whose effect on t is
              ln 2 times that, relative to t; 8 U covers the exp2 intrinsic (one ulp), the product with g and the adds; the
              last two are the error of S itself (d t / d S = t).  The G term adds 2 U |galpha G|; a floor of 1e-12 covers
              flushed denormals.  A bf16 dS adds 2^-7 |ref|: one ulp, nearest and truncating conversion alike.
  expsum      all addends are positive, so the bound is relative: sum_e exp(out_e) (bound(out_e) + 4 U)  (the error of the
              entry moved through exp, plus the exp2 intrinsic) + ACC_E expsum, ACC_E = (128 + 6 + 16 nob + 1) U: a lane
              adds at most 128 entries in sequence (4 tiles of 32), the wave sum 6 steps, 16 nob atomics per image and the
              dustbin column.
  score of gf_filter_matches   s (2 U |max0| + 8 U): __expf = exp2(x log2 e), one rounding of the argument and the intrinsic.
An arg-max is decided when the float64 gap between the best and the second best exceeds the sum of their value bounds."""
import functools
import math

import torch
import torch.nn.functional as F

from lg_loss_cases import GAP, Z_EDGES

TILE, OWNER, NSPLIT = 64, 128, 4
C_ACC, FLOOR = 1e-5, 1e-6
U = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
DETECT = 5.0              # a mutation must move an asserted output by this many bounds
MAX_BELOW_MARGIN = 1e-3   # share of rows of a `rand` case whose arg-max may be undecided

#          B  No    Ns
SHAPES = [(1, 1, 1), (2, 1, 65), (1, 64, 64), (3, 129, 63), (2, 300, 257), (3, 127, 449), (2, 130, 513), (1, 256, 1024)]
CONFIGS = [s + (256,) for s in SHAPES] + [s + (d,) for d in (64, 128) for s in SHAPES[3:]]      # (B, No, Ns, D)
DTYPES = [torch.float32, torch.bfloat16]
LARGE = ("first_dominates", "late_spike", "all_negative", "huge_bias")
KINDS = ("rand", "planted", "ties") + LARGE
# arg-max entries: (name, alpha, with bias); the bias of lse_argmax is logsigmoid(z) - nrm, that of argmax is sbias
ARG_VARIANTS = [("argmax", 1.0, False), ("argmax", 2.0, False), ("argmax", 1.0, True), ("argmax", 2.0, True),
                ("lse_argmax", 2.0, True)]


def split_ranges(Ns):
    """Row ranges [begin, end) of the streamed matrix that the four workgroups of a split kernel take (empty ones left out)."""
    per = -(-(-(-Ns // TILE)) // NSPLIT) * TILE
    return [(k * per, min(Ns, (k + 1) * per)) for k in range(NSPLIT) if k * per < Ns]


def special_rows(Ns, split):
    """Streamed rows at which a loop bound can be wrong: the first, the last, the first of a ragged last tile and, for the
    split kernels, the first and last of every split range."""
    rows = {0, Ns - 1}
    if Ns % TILE:
        rows.add(Ns // TILE * TILE)
    if split:
        for lo, hi in split_ranges(Ns):
            rows |= {lo, hi - 1}
    return sorted(rows)


def tie_pairs(Ns):
    """Disjoint (lowest, duplicate) index pairs: inside one lane's scan (3, 11: both in the lower half wave, g = 0 and 1), across
    the half waves with the lower index in the lower (1, 5) and in the upper half (6, 10) (offsets differing by 4), across
    tiles (2, 70), index 0 with Ns - 1 (the ragged last tile where there is one) and, where the ragged tile has a second
    row, from the last full tile to its first row."""
    cand = [(3, 11), (1, 5), (6, 10), (2, 70), (0, Ns - 1)]
    if Ns % TILE >= 2 and Ns > TILE:
        cand.append((Ns // TILE * TILE - 57, Ns // TILE * TILE))
    out, used = [], set()
    for lo, hi in cand:
        if 0 <= lo < hi < Ns and not {lo, hi} & used:
            out.append((lo, hi))
            used |= {lo, hi}
    return out


def has_kind(kind, Ns):
    return kind != "ties" or bool(tie_pairs(Ns))


# ----------------------------------------------------------------------------------------------- inputs
def _build(kind, B, No, Ns, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                   # noqa: E731
    case = {"kind": kind, "B": B, "No": No, "Ns": Ns, "D": D, "dtype": dtype, "seed": seed}
    bs = 3.0 if kind == "rand" else 1.0
    case.update(sbias=bs * rn(B, Ns), obias=bs * rn(B, No), z=rn(B, Ns), nrm=5.0 + rn(B, Ns), bin_s=rn(B, Ns), bin_o=rn(B, No),
                gr=rn(B, Ns), gc=rn(B, No), G=rn(B, Ns + 1, No + 1))
    if kind == "rand":                       # every image its own data (one draw over the batch)
        own, oth = 0.6 * rn(B, No, D), 0.6 * rn(B, Ns, D)
    else:
        s = math.sqrt(8.0 / D)
        oth = (s * rn(B, Ns, D)).to(dtype)
        win = torch.randint(0, Ns, (B, No), generator=g)
        if kind == "ties":
            pairs = tie_pairs(Ns)
            for lo, hi in pairs:
                oth[:, hi] = oth[:, lo]
                for k in ("sbias", "z", "nrm"):
                    case[k][:, hi] = case[k][:, lo]
            k = (torch.arange(No)[None] + torch.arange(B)[:, None]) % len(pairs)
            lo_t, hi_t = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
            win, case["tie_hi"] = lo_t[k], hi_t[k]
        else:                                # the first owner rows win at the rows where a loop bound can be wrong
            sp = torch.tensor(special_rows(Ns, False))[:B * No]
            win.view(-1)[:sp.numel()] = sp
        case["win"] = win
        own = 3.0 * oth.float().gather(1, win[..., None].expand(-1, -1, D)) + 0.3 * s * rn(B, No, D)
        oth = oth.float()
        if kind in ("first_dominates", "late_spike"):
            j = min(1, Ns - 1) if kind == "first_dominates" else Ns - 1
            oth[:, :, 0] = 0.0
            oth[:, j] = 0.0
            oth[:, j, 0] = 10.0
            own[:, :, 0] = 9.0 + 0.5 * torch.rand(B, No, generator=g)
            case["win"] = torch.full((B, No), j)
        elif kind == "all_negative":
            own[:, :, 0], oth[:, :, 0] = 10.0, -10.0
        elif kind == "huge_bias":
            e = min(Ns, len(Z_EDGES))
            case["z"][:, :e] = torch.tensor(Z_EDGES[:e])
    case["own"], case["oth"] = own.to(dtype), oth.to(dtype)
    if kind == "ties":                       # (the cast of equal rows is equal; written again so the property is plain)
        for lo, hi in tie_pairs(Ns):
            case["oth"][:, hi] = case["oth"][:, lo]
    S = case["own"].double() @ case["oth"].double().transpose(1, 2)
    case["r32"], case["c32"] = S.logsumexp(1).float(), S.logsumexp(2).float()      # normalisers of the backward, as fed (fp32)
    return case


def min_margin(case):
    """Smallest (gap - sum of the two value bounds) over the arg-max variants and rows, and the share of rows where it is
    negative.  For `ties` the duplicate is left out of the runners-up."""
    worst, below, rows = math.inf, 0, 0
    for v in ARG_VARIANTS:
        ref = ref_argmax(case, v)
        m = ref["gap"] - ref["bound_pair"]
        worst = min(worst, float(m.min()))
        below = max(below, int((m < 0).sum()))
        rows = m.numel()
    return worst, below / rows


@functools.lru_cache(maxsize=None)
def get_case(kind, B, No, Ns, D, dtype):
    """The case of a kind (module docstring of the tests for what each is for):
      rand             descriptors 0.6 randn (as the kernel tests' _head_inputs), biases 3 randn
      planted          oth = s randn, s = sqrt(8 / D); own_o = 3 oth_win(o) + 0.3 s randn: every owner row has a winner; the first
                       owner rows win at special_rows
      ties             planted, with the winning streamed row duplicated bit for bit (tie_pairs), biases included
      first_dominates  planted, and one streamed row of the first tile scores 90 .. 95 against every owner row
      late_spike       the same row as the last streamed row
      all_negative     planted with -100 added to every score
      huge_bias        planted with z = Z_EDGES on the first streamed rows
    Seeds are walked upward until every arg-max variant keeps a margin of GAP in float64, bias included, over the runner-up
    (`rand`: until at most MAX_BELOW_MARGIN of the rows are undecided).  Cached: the tensors are shared and must not be
    written to."""
    base = 1000 * B + 10 * No + Ns + D
    for seed in range(base, base + 200):
        case = _build(kind, B, No, Ns, D, dtype, seed)
        worst, share = min_margin(case)
        if (share <= MAX_BELOW_MARGIN) if kind == "rand" else (worst >= 0 and _min_gap(case) >= GAP):
            return case
    raise AssertionError(f"no seed gives {kind} {(B, No, Ns, D)} its margins")


def _min_gap(case):
    return min(float(ref_argmax(case, v)["gap"].min()) for v in ARG_VARIANTS)


def masked_bias(case):
    """sbias with -inf on every column of the last image: its rows have maximum -inf and index 0, as torch.max gives."""
    sb = case["sbias"].clone()
    sb[-1] = -math.inf
    return sb


# ----------------------------------------------------------------------------------------------- float64 references
def _scores(case, mut=None):
    """S [B,No,Ns], T_S (sum of |products|) and the multiplicity of every streamed row under the mutation."""
    shift = mut is not None and mut[0] == "owner_shift"
    key = "_S_shift" if shift else "_S"
    if key not in case:
        own, oth = case["own"].double(), case["oth"].double()
        if shift:
            own = own.roll(1, 1)
        S, T = own @ oth.transpose(1, 2), own.abs() @ oth.abs().transpose(1, 2)
        if "tie_hi" in case:                 # equal rows score equally; a blocked matrix product may add them in another order
            for lo, hi in tie_pairs(case["Ns"]):
                S[:, :, hi], T[:, :, hi] = S[:, :, lo], T[:, :, lo]
        case[key] = (S, T)
    w = torch.ones(case["Ns"], dtype=torch.float64)
    if mut is not None and mut[0] == "drop":
        w[list(mut[1])] = 0.0
    if mut is not None and mut[0] == "twice":
        w[mut[1]] = 2.0
    return case[key] + (w,)


def ref_lse(case, with_bias, mut=None, sbias=None):
    """lse[b,o] = log sum_s exp(S + sbias_s) and its bound.  Mutations: drop, twice, owner_shift, ln2_row."""
    S, TS, w = _scores(case, mut)
    X, TX = S, TS
    if with_bias:
        sb = (case["sbias"] if sbias is None else sbias).double()
        X, TX = S + sb[:, None, :], TS + sb.abs()[:, None, :]
    lse = (X + w.log()).logsumexp(2)
    if mut is not None and mut[0] == "ln2_row":
        lse = lse.clone()
        lse[-1, -1] += LN2
    T = TX.max(2).values + lse.abs()
    return {"lse": lse, "T": T, "bound": C_ACC * T + FLOOR}


def arg_parts(case, variant, sbias=None):
    name, _, with_bias = variant
    if name == "lse_argmax":
        return [F.logsigmoid(case["z"].double()), -case["nrm"].double()]
    return [(case["sbias"] if sbias is None else sbias).double()] if with_bias else []


def ref_argmax(case, variant, mut=None, sbias=None):
    """max / arg-max (lowest index of the maximum) over s of X = alpha S + bias, with the bound of every element of X (`bX`), the
    bound of the winner, the gap to the runner-up (for `ties`: to the best row that is not the duplicate) and the sum of
    the two bounds.  Mutations: drop, owner_shift, tile_local, tie_highest."""
    S, TS, w = _scores(case, mut)
    alpha = variant[1]
    X, TX = alpha * S, abs(alpha) * TS
    for p in arg_parts(case, variant, sbias):
        X, TX = X + p[:, None, :], TX + p.abs()[:, None, :]
    X = X.masked_fill(w == 0, -math.inf)
    val = X.max(2).values
    ar = torch.arange(case["Ns"])
    hit = X == val[..., None]
    first = torch.where(hit, ar, case["Ns"]).min(2).values
    idx = first
    if mut is not None and mut[0] == "tie_highest":
        idx = torch.where(hit, ar, -1).max(2).values
    if mut is not None and mut[0] == "tile_local":
        idx = idx % TILE
    bX = C_ACC * TX + FLOOR
    bX = torch.where(torch.isfinite(X), bX, torch.zeros_like(bX))
    Y = X.scatter(2, first[..., None], -math.inf)
    if "tie_hi" in case:
        Y = Y.scatter(2, case["tie_hi"][..., None], -math.inf)
    if case["Ns"] > 1 and torch.isfinite(Y).any():
        second, sidx = Y.max(2)
        gap = torch.where(torch.isfinite(val), val - second, torch.full_like(val, math.inf))
        b2 = bX.gather(2, sidx[..., None]).squeeze(2)
    else:
        gap, b2 = torch.full_like(val, math.inf), torch.zeros_like(val)
    bound = bX.gather(2, first[..., None]).squeeze(2)
    return {"val": val, "idx": idx, "X": X, "bX": bX, "bound": bound, "gap": gap, "bound_pair": bound + b2}


def swapped(case):
    """The case with owner and streamed matrix exchanged (S transposed): the lse over the OTHER axis."""
    return {"kind": case["kind"], "B": case["B"], "No": case["Ns"], "Ns": case["No"], "D": case["D"], "dtype": case["dtype"],
            "own": case["oth"], "oth": case["own"], "sbias": case["obias"], "obias": case["sbias"]}


def write_vecs(case, mode):
    """(rowbias [B,Ns], colbias [B,No], bin_col [B,Ns], bin_row [B,No]) of gf_assign_write, fp32:
      none   all four absent (None)
      plain  sbias, obias, bin_s, bin_o as drawn
      head   LightGlue's: logsig(z) - r, logsig(zo) - c, logsig(-z), logsig(-zo) with zo = bin_o and the fp32 normalisers; with
             alpha = 2 the matrix is a log assignment, its entries <= 0 and the dustbin column a visible share of expsum"""
    if mode == "none":
        return None
    if mode == "plain":
        return tuple(case[k] for k in ("sbias", "obias", "bin_s", "bin_o"))
    z, zo = case["z"], case["bin_o"]
    return (F.logsigmoid(z) - case["r32"], F.logsigmoid(zo) - case["c32"], F.logsigmoid(-z), F.logsigmoid(-zo))


def ref_write(case, alpha, corner, vecs, mut=None):
    """out [B,Ns+1,No+1] of gf_assign_write(a = oth, b = own) with vecs = (rowbias, colbias, bin_col, bin_row) (write_vecs; None:
    all four absent), its bound, expsum [B] and its bound.  Mutations: drop (the row stays unwritten: NaN), twice and
    no_dustbin (expsum), owner_shift."""
    S, TS, w = _scores(case, mut)
    B, No, Ns = case["B"], case["No"], case["Ns"]
    zero = lambda n: torch.zeros(B, n, dtype=torch.float64)                        # noqa: E731
    rb, cb, bc, br = (zero(Ns), zero(No), zero(Ns), zero(No)) if vecs is None else (v.double() for v in vecs)
    out = torch.zeros(B, Ns + 1, No + 1, dtype=torch.float64)
    T = torch.zeros_like(out)
    out[:, :Ns, :No] = alpha * S.transpose(1, 2) + rb[:, :, None] + cb[:, None, :]
    T[:, :Ns, :No] = abs(alpha) * TS.transpose(1, 2) + rb.abs()[:, :, None] + cb.abs()[:, None, :]
    out[:, :Ns, No], out[:, Ns, :No], out[:, Ns, No] = bc, br, corner
    T[:, :Ns, No], T[:, Ns, :No], T[:, Ns, No] = bc.abs(), br.abs(), abs(corner)
    bound = C_ACC * T + FLOOR
    e = out[:, :Ns].exp() * w[None, :, None]
    be = e * (bound[:, :Ns] + 4 * U)
    if mut is not None and mut[0] == "no_dustbin":
        e, be = e[:, :, :No], be[:, :, :No]
    expsum = e.sum((1, 2))
    acc_e = (128 + 6 + 16 * (-(-No // OWNER)) + 1) * U
    if mut is not None and mut[0] == "drop":
        out[:, list(mut[1]), :No] = math.nan
    return {"out": out, "T": T, "bound": bound, "expsum": expsum, "expsum_bound": be.sum((1, 2)) + acc_e * expsum}


def padded_G(case, ldg, fill=math.nan):
    """G [B,Ns+1,ldg] fp32: the case's G in [:, :Ns, :No], `fill` in the dustbin row, the dustbin column and the padding."""
    B, No, Ns = case["B"], case["No"], case["Ns"]
    G = torch.full((B, Ns + 1, ldg), fill, dtype=torch.float32)
    G[:, :Ns, :No] = case["G"][:, :Ns, :No]
    return G


def ref_bwd(case, with_G, galpha, out_dtype, mut=None):
    """dS [B,Ns,No] = galpha G + exp(S - r_s) gr_s + exp(S - c_o) gc_o of gf_dual_softmax_bwd(a = oth, b = own) on the stored fp32
    normalisers r32 / c32, with its bound and T (its three terms).  Mutations: drop (NaN), owner_shift, ldg_n (G read
    with a row stride of No), galpha_one, ln2_row."""
    S, TS, _ = _scores(case, mut)
    B, No, Ns = case["B"], case["No"], case["Ns"]
    St, TSt = S.transpose(1, 2), TS.transpose(1, 2)
    r, c = case["r32"].double(), case["c32"].double()
    if mut is not None and mut[0] == "ln2_row":
        r = r.clone()
        r[-1, -1] += LN2
    t2 = (St - r[:, :, None]).exp() * case["gr"].double()[:, :, None]
    t3 = (St - c[:, None, :]).exp() * case["gc"].double()[:, None, :]
    t1 = torch.zeros_like(t2)
    if with_G:
        G = padded_G(case, No + 1, 0.0).double()
        if mut is not None and mut[0] == "ldg_n":
            G = torch.as_strided(G.contiguous(), (B, Ns, No), ((Ns + 1) * (No + 1), No, 1))
        else:
            G = G[:, :Ns, :No]
        t1 = (1.0 if mut is not None and mut[0] == "galpha_one" else galpha) * G
    dS = t1 + t2 + t3
    es = C_ACC * TSt + FLOOR
    bound = (t2.abs() * (3 * U * (St.abs() + r.abs()[:, :, None]) + 8 * U + es)
             + t3.abs() * (3 * U * (St.abs() + c.abs()[:, None, :]) + 8 * U + es) + 2 * U * t1.abs() + 1e-12)
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -7 * dS.abs()
    if mut is not None and mut[0] == "drop":
        dS = dS.clone()
        dS[:, list(mut[1])] = math.nan
    return {"dS": dS, "T": t1.abs() + t2.abs() + t3.abs(), "bound": bound}


# ----------------------------------------------------------------------------------------------- fp32 rounding model
def model_scores(case):
    """S in fp32, the D products added one after the other (inputs as stored)."""
    if "_S32" not in case:
        own, oth = case["own"].float(), case["oth"].float()
        acc = torch.zeros(case["B"], case["No"], case["Ns"])
        for k in range(case["D"]):
            acc = acc + own[:, :, None, k] * oth[:, None, :, k]
        case["_S32"] = acc
    return case["_S32"]


_L2E = torch.tensor(LOG2E, dtype=torch.float32)
_LN2 = torch.tensor(LN2, dtype=torch.float32)


def model_lse(case, with_bias, sbias=None):
    x = model_scores(case) * _L2E
    if with_bias:
        x = x + ((case["sbias"] if sbias is None else sbias) * _L2E)[:, None, :]
    m = x.max(2).values
    return (m + torch.log2(torch.exp2(x - m[..., None]).sum(2))) * _LN2


def model_argmax(case, variant, sbias=None):
    name, alpha, with_bias = variant
    x = alpha * model_scores(case)
    if name == "lse_argmax":
        z = case["z"]
        x = x + (z.clamp(max=0.0) - torch.log1p(torch.exp(-z.abs())) - case["nrm"])[:, None, :]
    elif with_bias:
        x = x + (case["sbias"] if sbias is None else sbias)[:, None, :]
    val = x.max(2).values
    idx = torch.where(x == val[..., None], torch.arange(case["Ns"]), case["Ns"]).min(2).values
    return val, idx


def model_write(case, alpha, corner, vecs):
    B, No, Ns = case["B"], case["No"], case["Ns"]
    out = torch.zeros(B, Ns + 1, No + 1)
    core = alpha * model_scores(case).transpose(1, 2)
    if vecs is not None:
        core = core + vecs[0][:, :, None] + vecs[1][:, None, :]
        out[:, :Ns, No], out[:, Ns, :No] = vecs[2], vecs[3]
    out[:, :Ns, :No] = core
    out[:, Ns, No] = corner
    return out, torch.exp2(out[:, :Ns] * _L2E).sum((1, 2))


def model_bwd(case, with_G, galpha, out_dtype):
    x = model_scores(case).transpose(1, 2) * _L2E
    v = (torch.exp2(x - (case["r32"] * _L2E)[:, :, None]) * case["gr"][:, :, None]
         + torch.exp2(x - (case["c32"] * _L2E)[:, None, :]) * case["gc"][:, None, :])
    if with_G:
        v = v + galpha * case["G"][:, :case["Ns"], :case["No"]]
    return v.to(out_dtype)


# ----------------------------------------------------------------------------------------------- filter_matches
def filter_case():
    """(arg0, arg1, max0, la) of gf_filter_matches with B = 2, M = 5, N = 7, read off a hand-built log assignment la
    [B,M+1,N+1] (float64): a distinct background near -50 with planted entries -- mutual pairs above the threshold 0.1,
    mutual pairs below it ((3,3) and (3,5): exp = 0.018, 0.050), rows whose column prefers another row ((4,3), (4,5)),
    columns whose row prefers another column (the background), and in image 1 a row 0 and a column 0 of -inf: a mutual pair
    whose max0 is -inf, for th = 0.  No score lies within its bound of 0.1 or of 0."""
    B, M, N = 2, 5, 7
    i, j = torch.arange(M, dtype=torch.float64)[:, None], torch.arange(N, dtype=torch.float64)[None]
    la = (-50.0 - 0.37 * i - 0.05 * j - 0.011 * i * j).expand(B, M, N).clone()
    for b, r, c, v in ((0, 0, 2, -0.5), (0, 1, 0, -0.05), (0, 2, 6, -1.0), (0, 3, 3, -4.0), (0, 4, 3, -4.5),
                       (1, 1, 1, -0.01), (1, 2, 4, -0.3), (1, 3, 5, -3.0), (1, 4, 5, -3.5)):
        la[b, r, c] = v
    la[1, 0, :] = -math.inf
    la[1, :, 0] = -math.inf
    max0, arg0 = la.max(2)
    arg1 = la.max(1).indices
    full = torch.zeros(B, M + 1, N + 1, dtype=torch.float64)
    full[:, :M, :N] = la
    return arg0, arg1, max0.float(), full


def ref_filter(arg0, arg1, max0, th):
    """The mutual check in a few torch lines (float64) -> m0, m1, s0, s1 and the bounds of s0, s1."""
    max0 = max0.double()
    M, N = arg0.shape[1], arg1.shape[1]
    mut0 = arg1.gather(1, arg0) == torch.arange(M)[None]
    mut1 = arg0.gather(1, arg1) == torch.arange(N)[None]
    s0 = torch.where(mut0, max0.exp(), torch.zeros_like(max0))
    s1 = torch.where(mut1, s0.gather(1, arg1), torch.zeros(arg1.shape, dtype=torch.float64))
    m0 = torch.where(mut0 & (s0 > th), arg0, torch.full_like(arg0, -1))
    m1 = torch.where(mut1 & (s1 > th), arg1, torch.full_like(arg1, -1))
    ab = torch.where(torch.isfinite(max0), max0.abs(), torch.zeros_like(max0))
    b0 = s0 * (2 * U * ab + 8 * U)
    return m0, m1, s0, s1, b0, torch.where(mut1, b0.gather(1, arg1), torch.zeros_like(s1))
