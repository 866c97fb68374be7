"""Shared by tests/test_lg_loss_reference.py (CPU) and tests/test_gpu_lg_loss.py: float64 references of the fused LightGlue
layer loss (csrc/lg_loss.hip; contract in include/gf_amd.h) and the seeded inputs both files use.  No GPU code here.

Two references of the same sums:
  reference_dense  the full [B,M+1,N+1] log assignment (oracle.lightglue_oracle.log_double_softmax) and autograd;
  reference_stats  the sums from GIVEN statistics r, c, v0, a0, v1, a1 (plain data), with the closed-form gradients of
                   the header comment and, next to every value, the sum of the absolute values of its addends (`T`).
Descriptors are taken as stored: a bf16 tensor is upcast to float64, never rounded again.

`T` is what a float32 evaluation's rounding error is proportional to, so its addends are the ELEMENTARY ones of the
formulas: for a positive the D products of 2 md0_i.md1_j and the four statistics r_i, c_j, logsig(z0_i), logsig(z1_j)
(not the value A_ij, in which they may cancel); for a dustbin term neg * logsig(-z); for a BCE term max(t, 0), t * y and
log1p(exp(-|t|)); for a gradient its dense part and one term per positive that names the element."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle.lightglue_oracle import log_double_softmax

GAP = 2e-2            # smallest distance of any arg-max decision from its boundary that the inputs must keep
COO_P = 157           # length of the COO lists: no multiple of 4 (rows of a wave), 16 (a wave's chunk) or 64 (a block)

OPS_CASES = [(3, 70, 64), (2, 257, 256), (2, 130, 128)]                     # (B, N, D) of ops.lg_layer_loss
OPS_LISTS = ("fixed", "coo", "last_image", "all_skipped", "empty")
ABI_CASES = [(2, 37, 90, 36), (3, 1, 5, 4), (1, 300, 77, 200), (2, 64, 64, 68)]   # (B, M, N, D) of the C-ABI entries
ABI_LISTS = ("fixed", "coo", "empty")
Z_EDGES = (0.0, 30.0, -30.0, 90.0, -90.0)                                   # written into the first tokens of each image


def _f64(x):
    return None if x is None else x.double()


def _live(pos):
    pb, pi, pj = pos
    keep = pj >= 0
    return pb[keep], pi[keep], pj[keep]


def _counts(pos, B, M, N):
    """Multiplicity of every row of image 0 / image 1 in the list ([B,M], [B,N], float64)."""
    pb, pi, pj = _live(pos)
    one = torch.ones(pb.shape[0], dtype=torch.float64)
    c0 = torch.zeros(B * M, dtype=torch.float64).index_add_(0, pb * M + pi, one).view(B, M)
    c1 = torch.zeros(B * N, dtype=torch.float64).index_add_(0, pb * N + pj, one).view(B, N)
    return c0, c1


def _bce_terms(t, y):
    """The three addends of bce_with_logits(t, y) = max(t, 0) - t y + log1p(exp(-|t|))."""
    return t.clamp(min=0.0), -t * y, torch.log1p(torch.exp(-t.abs()))


def _top_gap(x):
    """(arg-max, largest minus second largest) along the last axis."""
    top = x.topk(2, dim=-1)
    return top.indices[..., 0], top.values[..., 0] - top.values[..., 1]


# ----------------------------------------------------------------------------------------------- dense reference
def reference_dense(md0, md1, z0, z1, t0, t1, pos, neg0, neg1, fin0, fin1):
    """acc [B,4] of one layer from the dense log assignment, all in float64 and differentiable in md0, md1, z0, z1, t0, t1.
    Positives count with their multiplicity, entries with pos_j < 0 are skipped, targets = (arg-max incl. dustbin == fin),
    detached.  Returns a dict: acc, tgt0 / tgt1 (None without fin), full0 / full1 (the arg-maxes incl. dustbin) and
    gap0 / gap1 (largest minus second-largest entry of every row / column, dustbin included)."""
    md0, md1, z0, z1, t0, t1 = (_f64(x) for x in (md0, md1, z0, z1, t0, t1))
    S = md0 @ md1.transpose(1, 2)
    la = log_double_softmax(S, z0, z1)
    B, M, N = S.shape
    pb, pi, pj = _live(pos)
    acc0 = torch.zeros(B, dtype=torch.float64).index_add(0, pb, la[pb, pi, pj])
    acc1 = (la[:, :M, N] * _f64(neg0)).sum(1) + (la[:, M, :N] * _f64(neg1)).sum(1)
    lad = la.detach()
    full0, gap0 = _top_gap(lad[:, :M, :])
    full1, gap1 = _top_gap(lad[:, :, :N].transpose(1, 2))
    tgt0 = None if fin0 is None else (full0 == fin0).double()
    tgt1 = None if fin1 is None else (full1 == fin1).double()
    acc2 = acc3 = torch.zeros(B, dtype=torch.float64)
    if t0 is not None:
        acc2 = F.binary_cross_entropy_with_logits(t0, tgt0, reduction="none").sum(1)
        acc3 = F.binary_cross_entropy_with_logits(t1, tgt1, reduction="none").sum(1)
    return {"acc": torch.stack([acc0, acc1, acc2, acc3], 1), "tgt0": tgt0, "tgt1": tgt1, "full0": full0, "full1": full1,
            "gap0": gap0, "gap1": gap1}


def dense_stats(md0, md1, z0, z1, r=None, c=None):
    """The statistics the loss kernels are fed with, in float64: r, c (row / column log-sum-exp of S, or the given ones),
    (v0, a0) = max / arg-max over j of 2 S_ij + logsig(z1_j) - c_j and (v1, a1) the same over i with z0 and r."""
    md0, md1, z0, z1 = (_f64(x.detach()) for x in (md0, md1, z0, z1))
    S = md0 @ md1.transpose(1, 2)
    r = S.logsumexp(2) if r is None else _f64(r)
    c = S.logsumexp(1) if c is None else _f64(c)
    v0, a0 = (2 * S + (F.logsigmoid(z1) - c)[:, None, :]).max(2)
    v1, a1 = (2 * S + (F.logsigmoid(z0) - r)[:, :, None]).max(1)
    return {"r": r, "c": c, "v0": v0, "a0": a0, "v1": v1, "a1": a1}


# ----------------------------------------------------------------------------------------------- reference on statistics
def reference_stats(md0, md1, z0, z1, t0, t1, pos, neg0, neg1, fin0, fin1, r, c, v0, a0, v1, a1, gacc=None):
    """The same sums from r, c, v0, a0, v1, a1 as plain data (float64 throughout):
      A_ij = 2 md0_i.md1_j - r_i - c_j + logsig(z0_i) + logsig(z1_j),  mx0 = v0 - r + logsig(z0),  mx1 = v1 - c + logsig(z1),
      target = ((bin > mx ? other : a) == fin)  with bin = logsig(-z), other = N for image 0 and M for image 1.
    With gacc [B,4] also the closed-form gradients: dz, dt, gr = -g count, gc = -g count (g = gacc[:,0], count = the
    multiplicity of the row in the list), and the sparse descriptor terms sp0[b,i] = sum 2 g md1[b,j],
    sp1[b,j] = sum 2 g md0[b,i].  Every value x comes with T_x, the sum of the absolute values of its addends; margin0 /
    margin1 are |bin - mx|, the distance of every target decision from its boundary; hits0 / hits1 the multiplicities."""
    md0, md1, z0, z1, t0, t1, neg0, neg1, r, c, v0, v1 = (
        None if x is None else _f64(x.detach()) for x in (md0, md1, z0, z1, t0, t1, neg0, neg1, r, c, v0, v1))
    B, M, D = md0.shape
    N = md1.shape[1]
    pb, pi, pj = _live(pos)
    lz0, lz1 = F.logsigmoid(z0), F.logsigmoid(z1)
    prod = md0[pb, pi] * md1[pb, pj]                                                  # [P, D]
    pieces = (r[pb, pi], c[pb, pj], lz0[pb, pi], lz1[pb, pj])
    A = 2 * prod.sum(1) - pieces[0] - pieces[1] + pieces[2] + pieces[3]
    TA = 2 * prod.abs().sum(1) + sum(x.abs() for x in pieces)
    zero = torch.zeros(B, dtype=torch.float64)
    acc0, T0 = zero.index_add(0, pb, A), zero.index_add(0, pb, TA)
    bin0, bin1 = F.logsigmoid(-z0), F.logsigmoid(-z1)
    acc1 = (bin0 * neg0).sum(1) + (bin1 * neg1).sum(1)
    T1 = (bin0 * neg0).abs().sum(1) + (bin1 * neg1).abs().sum(1)
    mx0, mx1 = v0 - r + lz0, v1 - c + lz1
    out = {"margin0": (bin0 - mx0).abs(), "margin1": (bin1 - mx1).abs(), "tgt0": None, "tgt1": None}
    full0 = torch.where(bin0 > mx0, torch.full_like(a0, N), a0)
    full1 = torch.where(bin1 > mx1, torch.full_like(a1, M), a1)
    out["full0"], out["full1"] = full0, full1
    if fin0 is not None:
        out["tgt0"], out["tgt1"] = (full0 == fin0).double(), (full1 == fin1).double()
    acc2 = acc3 = T2 = T3 = zero
    if t0 is not None:
        e0, e1 = _bce_terms(t0, out["tgt0"]), _bce_terms(t1, out["tgt1"])
        acc2, acc3 = sum(e0).sum(1), sum(e1).sum(1)
        T2, T3 = sum(x.abs() for x in e0).sum(1), sum(x.abs() for x in e1).sum(1)
    out["acc"], out["T_acc"] = torch.stack([acc0, acc1, acc2, acc3], 1), torch.stack([T0, T1, T2, T3], 1)
    cnt0, cnt1 = _counts(pos, B, M, N)
    out["hits0"], out["hits1"] = cnt0, cnt1
    if gacc is None:
        return out
    gacc = _f64(gacc)
    g, gneg = gacc[:, 0:1], gacc[:, 1:2]
    for k, z, neg, cnt in (("0", z0, neg0, cnt0), ("1", z1, neg1, cnt1)):
        dense, sparse = -gneg * neg * torch.sigmoid(z), g * cnt * torch.sigmoid(-z)
        out["dz" + k], out["T_dz" + k] = dense + sparse, dense.abs() + sparse.abs()
        out["g" + ("r" if k == "0" else "c")] = -g * cnt
    if t0 is not None:
        for k, t, col in (("0", t0, 2), ("1", t1, 3)):
            gb = gacc[:, col:col + 1]
            out["dt" + k] = gb * (torch.sigmoid(t) - out["tgt" + k])
            out["T_dt" + k] = gb.abs() * (torch.sigmoid(t) + out["tgt" + k])
    g2 = 2 * gacc[pb, 0][:, None]
    z0f, z1f = torch.zeros(B * M, D, dtype=torch.float64), torch.zeros(B * N, D, dtype=torch.float64)
    out["sp0"] = z0f.index_add(0, pb * M + pi, g2 * md1[pb, pj]).view(B, M, D)
    out["T_sp0"] = z0f.index_add(0, pb * M + pi, (g2 * md1[pb, pj]).abs()).view(B, M, D)
    out["sp1"] = z1f.index_add(0, pb * N + pj, g2 * md0[pb, pi]).view(B, N, D)
    out["T_sp1"] = z1f.index_add(0, pb * N + pj, (g2 * md0[pb, pi]).abs()).view(B, N, D)
    return out


# ----------------------------------------------------------------------------------------------- positives lists
def _batch_rows(B, n):
    return torch.arange(B).repeat_interleave(n), torch.arange(n).repeat(B)


def _coo_list(pairs, B, M, N, P, g):
    """A COO list of exactly P entries in random order: distinct pairs (the given ones shuffled across images, topped up
    with random pairs where they are too few), 5 of them listed twice, and 3 more pairs on one column of md1 (from 3
    further rows of that image where it has them; a one-row image repeats its row)."""
    pb, pi, pj = pairs
    base = P - 8
    order = torch.randperm(pb.shape[0], generator=g)[:base]
    pb, pi, pj = pb[order], pi[order], pj[order]
    seen = {(int(b), int(i), int(j)) for b, i, j in zip(pb, pi, pj)}
    extra = []
    while len(seen) < base:
        e = (int(torch.randint(B, (1,), generator=g)), int(torch.randint(M, (1,), generator=g)),
             int(torch.randint(N, (1,), generator=g)))
        if e not in seen:
            seen.add(e)
            extra.append(e)
    if extra:
        eb, ei, ej = (torch.tensor(x, dtype=torch.int64) for x in zip(*extra))
        pb, pi, pj = torch.cat([pb, eb]), torch.cat([pi, ei]), torch.cat([pj, ej])
    dup = torch.randperm(base, generator=g)[:5]
    b_, i_, j_ = int(pb[0]), int(pi[0]), int(pj[0])
    others = [i for i in torch.randperm(M, generator=g).tolist() if i != i_][:3]
    others += [i_] * (3 - len(others))
    pb = torch.cat([pb, pb[dup], torch.full((3,), b_, dtype=torch.int64)])
    pi = torch.cat([pi, pi[dup], torch.tensor(others, dtype=torch.int64)])
    pj = torch.cat([pj, pj[dup], torch.full((3,), j_, dtype=torch.int64)])
    order = torch.randperm(P, generator=g)
    assert pb.shape[0] == P
    return pb[order], pi[order], pj[order]


def positives(case, kind):
    """(pos_b, pos_i, pos_j) int64 CPU vectors of a case (planted_case or abi_case):
      fixed        one slot per row of image 0, sorted by image, -1 where the row has no positive
      coo          see _coo_list; P = case["coo_P"]
      last_image   the fixed list with every slot outside image B-1 set to -1
      all_skipped  the fixed list with every slot set to -1
      empty        P = 0"""
    B, M, N = case["B"], case["M"], case["N"]
    match = case["match"]                                                             # [B,M]: partner or -1
    pb, pi = _batch_rows(B, M)
    if kind == "fixed":
        return pb, pi, match.reshape(-1).clone()
    if kind == "last_image":
        return pb, pi, torch.where(pb == B - 1, match.reshape(-1), torch.full((B * M,), -1))
    if kind == "all_skipped":
        return pb, pi, torch.full((B * M,), -1)
    if kind == "empty":
        e = torch.zeros(0, dtype=torch.int64)
        return e, e.clone(), e.clone()
    assert kind == "coo"
    keep = match.reshape(-1) >= 0
    g = torch.Generator().manual_seed(7000 + case["seed"] + 10 * M + N)
    return _coo_list((pb[keep], pi[keep], match.reshape(-1)[keep]), B, M, N, case["coo_P"], g)


# ----------------------------------------------------------------------------------------------- planted case (ops level)
def _move_half(full, other, g):
    """`full` with a seeded random half of the entries of every image moved to a different index in [0, other]; one moved
    entry per image whose arg-max is a keypoint is moved to the dustbin, so that the dustbin is on the disagreeing side too."""
    B, n = full.shape
    moved = torch.zeros(B, n, dtype=torch.bool)
    for b in range(B):
        if n > 1:
            moved[b, torch.randperm(n, generator=g)[:n // 2]] = True
        else:                                                                         # a one-token image: a coin per image
            moved[b, 0] = bool(torch.rand(1, generator=g) < 0.5)
    off =torch.randint(1, other + 1, (B, n), generator=g)
    fin = torch.where(moved, (full + off) % (other + 1), full)
    for b in range(B):
        k = (moved[b] & (full[b] != other)).nonzero()
        if k.numel():
            fin[b, k[0, 0]] = other
    return fin


def _planted(B, N, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    s = math.sqrt(8.0 / D)
    md0 = torch.randn(B, N, D, generator=g) * s
    md1 = torch.randn(B, N, D, generator=g) * s
    noise = torch.randn(B, N, D, generator=g)
    match = torch.full((B, N), -1, dtype=torch.int64)
    for b in range(B):
        rows = torch.randperm(N, generator=g)[:N // 2]
        match[b, rows] = torch.randperm(N, generator=g)[rows]
    bi, ii = (match >= 0).nonzero(as_tuple=True)
    jj = match[bi, ii]
    md1[bi, jj] = md0[bi, ii] + 0.1 * s * noise[bi, ii]
    has1 = torch.zeros(B, N, dtype=torch.bool)
    has1[bi, jj] = True
    z0 = torch.where(match >= 0, 3.0, -3.0) + torch.randn(B, N, generator=g)
    z1 = torch.where(has1, 3.0, -3.0) + torch.randn(B, N, generator=g)
    case = {"B": B, "M": N, "N": N, "D": D, "seed": seed, "coo_P": COO_P, "match": match,
            "md0": md0.to(dtype), "md1": md1.to(dtype), "z0": z0, "z1": z1,
            "t0": 1.5 * torch.randn(B, N, generator=g), "t1": 1.5 * torch.randn(B, N, generator=g),
            "neg0": (match < 0).float(), "neg1": (~has1).float(), "gacc": torch.randn(B, 4, generator=g)}
    e = torch.zeros(0, dtype=torch.int64)
    ref = reference_dense(case["md0"], case["md1"], z0, z1, None, None, (e, e, e), case["neg0"], case["neg1"], None, None)
    case["full0"], case["full1"], case["gap0"], case["gap1"] = ref["full0"], ref["full1"], ref["gap0"], ref["gap1"]
    case["fin0"], case["fin1"] = _move_half(ref["full0"], N, g), _move_half(ref["full1"], N, g)
    return case


@functools.lru_cache(maxsize=None)
def planted_case(B, N, D, dtype, seed=0):
    """Inputs of ops.lg_layer_loss with planted matches (with plain random descriptors the dustbin wins nearly every
    arg-max and the a[base + i] branch of the target would go untested): md0 = randn s with s = sqrt(8 / D); a random half
    of the tokens of image 0 is matched, md1[perm[i]] = md0[i] + 0.1 s randn for those and randn s elsewhere;
    z = +3 + randn on matched tokens and their partners, -3 + randn elsewhere; then the cast to `dtype`.  fin0 / fin1 are the
    float64 arg-maxes with a random half moved (_move_half).  Seeds are walked upward from `seed` until every row and
    column of the float64 log assignment OF THE STORED VALUES has a top-2 gap of at least GAP; the case carries the seed
    it settled on.  Cached: the tensors are shared between tests and must not be written to."""
    for sd in range(seed, seed + 50):
        case = _planted(B, N, D, dtype, sd)
        if min(float(case["gap0"].min()), float(case["gap1"].min())) >= GAP:
            return case
    raise AssertionError("no seed gives every row and column a top-2 gap of GAP")


# ----------------------------------------------------------------------------------------------- stated statistics (C ABI)
def abi_P(B, M, N):
    """Largest P up to COO_P that B M N distinct pairs allow and that is no multiple of 4."""
    p = min(COO_P, B * M * N)
    while p % 4 == 0:
        p -= 1
    return p


def _stated_side(z, nrm, n_other, g):
    """(v, a, fin) of one image: a seeded, v = mx + nrm - logsig(z) (rounded to fp32) for an mx placed at a seeded distance
    of at least 0.05 on a seeded side of bin = logsig(-z), fin = the resulting arg-max incl. dustbin with half moved."""
    zd, nd = z.double(), nrm.double()
    lz = F.logsigmoid(zd)
    delta = (0.05 + 0.5 * torch.randn(z.shape, generator=g).abs()) * torch.where(torch.rand(z.shape, generator=g) < 0.5, -1.0, 1.0)
    v = ((lz - zd) + delta + nd - lz).float()
    a = torch.randint(0, n_other, z.shape, generator=g)
    full = torch.where(delta < 0, torch.full_like(a, n_other), a)
    return v, a, _move_half(full, n_other, g)


@functools.lru_cache(maxsize=None)
def abi_case(B, M, N, D, dtype, seed=0):
    """Inputs of the three C-ABI entries with STATED statistics (r, c, v, a are seeded arrays, not derived from the
    descriptors): md = randn sqrt(1.5 / sqrt(D)) cast to `dtype`; z seeded normal with Z_EDGES written into the first
    tokens of each image (as many as the image has); r, c ~ N(5, 1); v such that |bin - mx| >= 0.05 before its rounding to
    fp32 (the CPU test holds the stored values to GAP); fin with about half of the targets 1; real-valued dustbin weights;
    a dyadic gacc (k / 64, |k| in 1..127), so that -g count is exact in fp32 in whatever order the atomics land.
    Cached: the tensors are shared between tests and must not be written to."""
    g = torch.Generator().manual_seed(31000 + seed + 1000 * B + 10 * M + N + D)
    s = math.sqrt(1.5 / math.sqrt(D))
    case = {"B": B, "M": M, "N": N, "D": D, "seed": seed, "coo_P": abi_P(B, M, N), "scale": s,
            "md0": (torch.randn(B, M, D, generator=g) * s).to(dtype), "md1": (torch.randn(B, N, D, generator=g) * s).to(dtype)}
    for k, n in (("0", M), ("1", N)):
        z = torch.randn(B, n, generator=g)
        e = min(n, len(Z_EDGES))
        z[:, :e] = torch.tensor(Z_EDGES[:e])
        case["z" + k] = z
        case["t" + k] = 2.0 * torch.randn(B, n, generator=g)
        case["neg" + k] = torch.rand(B, n, generator=g)
    case["r"], case["c"] = 5.0 + torch.randn(B, M, generator=g), 5.0 + torch.randn(B, N, generator=g)
    case["v0"], case["a0"], case["fin0"] = _stated_side(case["z0"], case["r"], N, g)
    case["v1"], case["a1"], case["fin1"] = _stated_side(case["z1"], case["c"], M, g)
    match = torch.randint(0, N, (B, M), generator=g)
    match[torch.rand(B, M, generator=g) < 0.4] = -1
    if M * B > 1:
        match.view(-1)[0] = 0                                                        # at least one live and one skipped slot
        match.view(-1)[-1] = -1
    case["match"] = match
    k = torch.randint(1, 128, (B, 4), generator=g) * torch.where(torch.rand(B, 4, generator=g) < 0.5, -1, 1)
    case["gacc"] = k.float() / 64.0
    case["base0"] = (torch.randn(B, M, D, generator=g) * s).to(dtype)
    case["base1"] = (torch.randn(B, N, D, generator=g) * s).to(dtype)
    return case


def stats_of(case, pos, with_t=True, gacc=True):
    """reference_stats of an abi_case on its stated statistics."""
    t0, t1 = (case["t0"], case["t1"]) if with_t else (None, None)
    return reference_stats(case["md0"], case["md1"], case["z0"], case["z1"], t0, t1, pos, case["neg0"], case["neg1"],
                           case["fin0"], case["fin1"], case["r"], case["c"], case["v0"], case["a0"], case["v1"], case["a1"],
                           case["gacc"] if gacc else None)
