"""Sparse positives of the NLL losses: one gradient write, its row / column sums handed to the consumers."""
import weakref

import torch


# ------------------------------------------------------------------------------ sparse positives of the NLL losses
_SPARSE_SUMS = {}        # data_ptr of the dense gradient _NllTerms just wrote -> (weakref, row sums, column sums)


def _known_sums(G):
    hit = _SPARSE_SUMS.pop(G.data_ptr(), None)
    if (hit is not None and hit[0]() is G and hit[4] == G._version and hit[1].shape == G.shape[:2]
            and hit[2].shape == (G.shape[0], G.shape[2])):
        return hit[1].contiguous(), hit[2].contiguous()
    return None


def _known_sparse(G):
    """(col index of each row's positive, its gradient value (0 where none), dustbin-column values, dustbin-row values) when
    G is the gradient _NllTerms just wrote (so: nothing else anywhere), else None."""
    hit = _SPARSE_SUMS.pop(G.data_ptr(), None)
    if hit is not None and hit[0]() is G and hit[4] == G._version and hit[3][0].shape == (G.shape[0], G.shape[1] - 1):
        return hit[3]
    return None


class _NllTerms(torch.autograd.Function):
    """(sum over the positives of la[b, i, col0[b, i]], sum over the unmatched rows / columns of their dustbin entries) of a
    log assignment la [B, M+1, N+1] (superglue.py:322-352, gluestick.py:378-414).  The gradient is written ONCE: one fill of
    the dense matrix + three sparse writes -- autograd's own backward of the gather and the two dustbin slices builds three
    dense tensors and adds them (1.4 ms per SuperGlue step at 32 x 2049^2)."""

    @staticmethod
    def forward(ctx, la, col0, neg0, neg1):
        valid = col0 >= 0
        idx = col0.clamp(min=0).long()[..., None]
        picked = la[:, :-1, :].gather(2, idx).squeeze(-1)
        pos = (picked * valid.to(picked.dtype)).sum(1)
        neg = (la[:, :-1, -1] * neg0).sum(1) + (la[:, -1, :-1] * neg1).sum(1)
        ctx.save_for_backward(idx, valid, neg0, neg1)
        ctx.shape, ctx.dtype = la.shape, la.dtype
        return pos, neg

    @staticmethod
    def backward(ctx, gpos, gneg):
        idx, valid, neg0, neg1 = ctx.saved_tensors
        G = torch.zeros(ctx.shape, dtype=ctx.dtype, device=idx.device)
        vpos = gpos[:, None] * valid.to(ctx.dtype)
        n0, n1 = gneg[:, None] * neg0, gneg[:, None] * neg1
        G[:, :-1, :].scatter_(2, idx, vpos[..., None])
        G[:, :-1, -1] = n0                               # (a positive never sits in the dustbin column)
        G[:, -1, :-1] = n1
        # row / column sums of this sparse matrix, for a consumer that wants them (the Sinkhorn backward): known here
        # from O(M + N) values instead of two more sweeps of the dense tensor
        gr = torch.cat([vpos + n0, n1.sum(1, keepdim=True)], 1)
        gc = torch.cat([n1, n0.sum(1, keepdim=True)], 1).scatter_add_(1, idx.squeeze(-1), vpos)
        _SPARSE_SUMS.clear()
        # G._version: autograd's input buffer ACCUMULATES a second gradient of the same tensor in place (version bump) --
        # the sparse description would then be incomplete, and the consumers fall back to the dense tensor
        _SPARSE_SUMS[G.data_ptr()] = (weakref.ref(G), gr, gc, (idx.squeeze(-1), vpos, n0, n1), G._version)
        return G, None, None, None


def nll_terms(la, data, neg0, neg1, prefix=""):
    """-> (sum of la over the positives, number of positives, sum of the dustbin entries of the unmatched rows and columns),
    per pair.  With the ground truth's ``gt_<prefix>assignment_col0`` vector: one autograd node (see _NllTerms)."""
    col0 = data.get("gt_" + prefix + "assignment_col0")
    if col0 is not None:
        pos, neg = _NllTerms.apply(la, col0, neg0, neg1)
        return pos, (col0 >= 0).sum(1).float(), neg
    pos, num_pos = nll_positive_terms(la, data, prefix)
    return pos, num_pos, (la[:, :-1, -1] * neg0).sum(1) + (la[:, -1, :-1] * neg1).sum(1)


def nll_positive_terms(la, data, prefix=""):
    """(sum over the positives of la[b,i,j], number of positives) per pair, for the NLL of superglue.py:322-352 and
    gluestick.py:378-414 (weights = gt_assignment).  When the ground-truth producer supplied
    ``gt_<prefix>assignment_col0`` (the single positive column of each row, -1 if none: ours do) the terms are one
    fixed-length gather -- no scan of the dense matrix, no host synchronisation, capturable in a hipGraph; otherwise
    the dense matrix is scanned with nonzero() (same numbers, one host read)."""
    bsz = la.shape[0]
    col0 = data.get("gt_" + prefix + "assignment_col0")
    if col0 is not None:
        valid = col0 >= 0
        picked = la[:, :-1, :].gather(2, col0.clamp(min=0).long()[..., None]).squeeze(-1)
        return (picked * valid.to(picked.dtype)).sum(1), valid.sum(1).float()
    bi, ii, ji = data["gt_" + prefix + "assignment"].nonzero(as_tuple=True)
    zeros = torch.zeros(bsz, device=la.device)
    return zeros.index_add(0, bi, la[bi, ii, ji]), zeros.index_add(0, bi, torch.ones_like(bi, dtype=torch.float32))
