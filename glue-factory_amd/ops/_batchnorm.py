"""BatchNorm1d (+ReLU) nodes, SyncBatchNorm exchange and running-statistics replay (csrc/batchnorm.hip)."""
import torch

from .. import lib as _lib
from ._base import _chk, _dt, _p, _stream


# ------------------------------------------------------------------------------ BatchNorm1d (+ReLU)
class _BatchNormAct(torch.autograd.Function):
    """act(BatchNorm(x)) on channels-last x [M,C]; batch statistics in training (optionally summed
    across ranks = SyncBatchNorm), given statistics in eval.  Returns (y, mean, biased var, count);
    only y is differentiable."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean_in, rstd_in, eps, training, relu, sync, run_mean=None, run_var=None,
                momentum=0.0):
        """run_mean / run_var (fp32, contiguous) given: updated in place by the finalize kernel (single-process
        training); otherwise the caller updates the running statistics from the returned mean / var / n."""
        _chk(x)
        M, C = x.shape
        L = _lib.load()
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        if training:
            nblk = L.gf_bn_nblk(M)
            part = torch.empty((nblk, 2, C), dtype=torch.float32, device=x.device)
            _lib.check(L.gf_bn_stats(_p(x), _p(part), M, C, _dt(x), _stream()), "gf_bn_stats")
            if sync:
                import torch.distributed as dist
                s = part.sum(0)
                n_t = torch.full((), float(M), dtype=s.dtype, device=s.device)      # device-side fill: capturable
                packed = torch.cat([s.flatten(), n_t[None]])
                dist.all_reduce(packed)
                s, n_t = packed[:-1].view(2, C), packed[-1]
                mean = (s[0] / n_t).contiguous()
                var = (s[1] / n_t - mean * mean).clamp(min=0.0)
                rstd = torch.rsqrt(var + eps).contiguous()
            else:       # one kernel: block sums -> mean / var / rstd (+ running statistics)
                mvr = torch.empty((3, C), dtype=torch.float32, device=x.device)
                mean, var, rstd = mvr[0], mvr[1], mvr[2]
                _lib.check(L.gf_bn_finalize_fwd(_p(part), nblk, C, float(M), float(eps), float(momentum), _p(mean),
                                                _p(var), _p(rstd), _p(run_mean), _p(run_var), _stream()),
                           "gf_bn_finalize_fwd")
                n_t = float(M)
        else:
            mean, rstd = mean_in.float().contiguous(), rstd_in.float().contiguous()
            var, n_t = mean.new_zeros(C), float(M)
        y = torch.empty_like(x)
        _lib.check(L.gf_bn_act_fwd(_p(x), _p(mean), _p(rstd), _p(g32), _p(b32), _p(y), M, C, int(relu), _dt(x),
                                   _stream()), "gf_bn_act_fwd")
        if torch.is_tensor(n_t):
            ctx.save_for_backward(x, mean, rstd, g32, b32, n_t)
            ctx.n = None
        else:
            ctx.save_for_backward(x, mean, rstd, g32, b32)
            ctx.n = n_t
            n_t = torch.empty(0, device=x.device)          # placeholder output (the count is a host constant here)
        ctx.cfg = (training, relu, sync, gamma.dtype, beta.dtype)
        ctx.mark_non_differentiable(mean, var, n_t)
        return y, mean, var, n_t

    @staticmethod
    def backward(ctx, dy, _gm, _gv, _gn):
        if ctx.n is None:
            x, mean, rstd, g32, b32, n_t = ctx.saved_tensors
        else:
            x, mean, rstd, g32, b32 = ctx.saved_tensors
            n_t = None
        training, relu, sync, gdt, bdt = ctx.cfg
        M, C = x.shape
        if not dy.is_contiguous():
            dy = dy.contiguous()
        L = _lib.load()
        nblk = L.gf_bn_nblk(M)
        part = torch.empty((nblk, 2, C), dtype=torch.float32, device=x.device)
        _lib.check(L.gf_bn_bwd_stats(_p(x), _p(dy), _p(mean), _p(rstd), _p(g32), _p(b32), _p(part), M, C,
                                     int(relu), _dt(x), _stream()), "gf_bn_bwd_stats")
        if training and not sync:
            out = torch.empty((4, C), dtype=torch.float32, device=x.device)
            dbeta, dgamma, m1, m2 = out[0], out[1], out[2], out[3]
            _lib.check(L.gf_bn_finalize_bwd(_p(part), nblk, C, float(M), _p(dbeta), _p(dgamma), _p(m1), _p(m2),
                                            _stream()), "gf_bn_finalize_bwd")
        else:
            s = part.sum(0)
            dbeta, dgamma = s[0].clone(), s[1].clone()          # local sums: DDP averages parameter grads
            if training:
                import torch.distributed as dist
                s = s.contiguous()
                dist.all_reduce(s)
                m1, m2 = (s[0] / n_t).contiguous(), (s[1] / n_t).contiguous()
            else:
                m1 = m2 = torch.zeros(C, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        _lib.check(L.gf_bn_bwd_dx(_p(x), _p(dy), _p(mean), _p(rstd), _p(g32), _p(b32), _p(m1), _p(m2), _p(dx),
                                  M, C, int(relu), _dt(x), _stream()), "gf_bn_bwd_dx")
        return dx, dgamma.to(gdt), dbeta.to(bdt), None, None, None, None, None, None, None, None, None


class _BatchNormActSets(torch.autograd.Function):
    """act(BatchNorm(x[h])) for h = 0..H-1 on x [H,M,C]: H independent statistics sets through the SAME BatchNorm
    module (the reference calls its MLP once per image: superglue.py:70-79 via :276-283), single-process training.
    One node: no select / stack copies around the per-image calls, running statistics updated set after set."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, run_mean, run_var, momentum, replay=None):
        """replay: None, or the module's num_batches_tracked buffer -- the BACKWARD then applies the H running-statistics
        updates a second time (gf_bn_replay_running) and counts them, as an activation-checkpointed reference does when its
        backward re-runs the forward in training mode (superglue.py:160-169; gluestick.py:724-757 with `checkpointed`)."""
        _chk(x)
        H, M, C = x.shape
        L = _lib.load()
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        nblk = L.gf_bn_nblk(M)
        part = torch.empty((nblk, 2, C), dtype=torch.float32, device=x.device)
        mvr = torch.empty((H, 3, C), dtype=torch.float32, device=x.device)
        ctx.replay = None if replay is None else (run_mean, run_var, replay, float(momentum))
        y = torch.empty_like(x)
        st, dt = _stream(), _dt(x)
        for h in range(H):
            _lib.check(L.gf_bn_stats(_p(x[h]), _p(part), M, C, dt, st), "gf_bn_stats")
            _lib.check(L.gf_bn_finalize_fwd(_p(part), nblk, C, float(M), float(eps), float(momentum), _p(mvr[h, 0]),
                                            _p(mvr[h, 1]), _p(mvr[h, 2]), _p(run_mean), _p(run_var), st),
                       "gf_bn_finalize_fwd")
            _lib.check(L.gf_bn_act_fwd(_p(x[h]), _p(mvr[h, 0]), _p(mvr[h, 2]), _p(g32), _p(b32), _p(y[h]), M, C,
                                       int(relu), dt, st), "gf_bn_act_fwd")
        ctx.save_for_backward(x, mvr, g32, b32)
        ctx.cfg = (relu, gamma.dtype, beta.dtype)
        ctx.mark_non_differentiable(mvr)
        return y, mvr

    @staticmethod
    def backward(ctx, dy, _gmvr):
        x, mvr, g32, b32 = ctx.saved_tensors
        relu, gdt, bdt = ctx.cfg
        H, M, C = x.shape
        if not dy.is_contiguous():
            dy = dy.contiguous()
        L = _lib.load()
        nblk = L.gf_bn_nblk(M)
        part = torch.empty((nblk, 2, C), dtype=torch.float32, device=x.device)
        out = torch.empty((H, 4, C), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        st, dt = _stream(), _dt(x)
        for h in range(H):
            mean, rstd = mvr[h, 0], mvr[h, 2]
            _lib.check(L.gf_bn_bwd_stats(_p(x[h]), _p(dy[h]), _p(mean), _p(rstd), _p(g32), _p(b32), _p(part), M, C,
                                         int(relu), dt, st), "gf_bn_bwd_stats")
            _lib.check(L.gf_bn_finalize_bwd(_p(part), nblk, C, float(M), _p(out[h, 0]), _p(out[h, 1]), _p(out[h, 2]),
                                            _p(out[h, 3]), st), "gf_bn_finalize_bwd")
            _lib.check(L.gf_bn_bwd_dx(_p(x[h]), _p(dy[h]), _p(mean), _p(rstd), _p(g32), _p(b32), _p(out[h, 2]),
                                      _p(out[h, 3]), _p(dx[h]), M, C, int(relu), dt, st), "gf_bn_bwd_dx")
        dbeta, dgamma = (out[0, 0], out[0, 1]) if H == 1 else (out[:, 0].sum(0), out[:, 1].sum(0))
        if ctx.replay is not None:
            run_mean, run_var, nbt, momentum = ctx.replay
            from . import REPLAY_GATE       # the package attribute, read at call time: TrainStep rebinds it around its backward
            gate = REPLAY_GATE
            _lib.check(L.gf_bn_replay_running(_p(mvr), H, C, float(M), momentum, _p(run_mean), _p(run_var), _p(gate), st),
                       "gf_bn_replay_running")
            nbt.add_(H if gate is None else (gate == 0).to(nbt.dtype) * H)
        return dx, dgamma.to(gdt), dbeta.to(bdt), None, None, None, None, None, None


COLLECTIVES = {"syncbn": 0}       # collectives issued by the ops of this module (bench.py / tests count them per step)


def _all_reduce_sum(t):
    import torch.distributed as dist
    COLLECTIVES["syncbn"] += 1
    dist.all_reduce(t)


class _BatchNormActSetsSync(torch.autograd.Function):
    """_BatchNormActSets under SyncBatchNorm (train.py:338): the H statistics sets of a call -- both images through the SAME
    BatchNorm module (superglue.py:70-79 via :276-283) -- share ONE all-reduce per direction instead of one per set: the block
    sums of all sets are packed with their row counts (gf_bn_pack_sums), reduced across ranks, and the fused finalize kernels
    read the reduced buffer (mean / var / rstd of every set + the running statistics, set after set; m1 / m2 in the backward).
    Row counts may differ between ranks (they are reduced with the sums).  dgamma / dbeta stay LOCAL sums: the gradient reducer
    averages parameter gradients across ranks."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, run_mean, run_var, momentum, replay=None):
        _chk(x)
        H, M, C = x.shape
        L = _lib.load()
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        nblk = L.gf_bn_nblk(M)
        part = torch.empty((H, nblk, 2, C), dtype=torch.float32, device=x.device)
        packed = torch.empty(H * 2 * C + H, dtype=torch.float32, device=x.device)
        mvr = torch.empty((H, 3, C), dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        st, dt = _stream(), _dt(x)
        for h in range(H):
            _lib.check(L.gf_bn_stats(_p(x[h]), _p(part[h]), M, C, dt, st), "gf_bn_stats")
        _lib.check(L.gf_bn_pack_sums(_p(part), H, nblk, C, float(M), _p(packed), None, st), "gf_bn_pack_sums")
        _all_reduce_sum(packed)                                   # ONE exchange for the H sets
        _lib.check(L.gf_bn_finalize_sets_fwd(_p(packed), H, C, float(eps), float(momentum), _p(mvr), _p(run_mean), _p(run_var),
                                             st), "gf_bn_finalize_sets_fwd")
        counts = packed[H * 2 * C:]                               # the reduced row count of every set
        for h in range(H):
            _lib.check(L.gf_bn_act_fwd(_p(x[h]), _p(mvr[h, 0]), _p(mvr[h, 2]), _p(g32), _p(b32), _p(y[h]), M, C,
                                       int(relu), dt, st), "gf_bn_act_fwd")
        ctx.replay = None if replay is None else (run_mean, run_var, replay, float(momentum))
        ctx.save_for_backward(x, mvr, g32, b32, counts)
        ctx.cfg = (relu, gamma.dtype, beta.dtype)
        ctx.mark_non_differentiable(mvr, counts)
        return y, mvr, counts

    @staticmethod
    def backward(ctx, dy, _gmvr, _gc):
        x, mvr, g32, b32, counts = ctx.saved_tensors
        relu, gdt, bdt = ctx.cfg
        H, M, C = x.shape
        if not dy.is_contiguous():
            dy = dy.contiguous()
        L = _lib.load()
        nblk = L.gf_bn_nblk(M)
        part = torch.empty((H, nblk, 2, C), dtype=torch.float32, device=x.device)
        packed = torch.empty(H * 2 * C + H, dtype=torch.float32, device=x.device)
        local = torch.empty((H, 2, C), dtype=torch.float32, device=x.device)
        m12 = torch.empty((H, 2, C), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        st, dt = _stream(), _dt(x)
        for h in range(H):
            _lib.check(L.gf_bn_bwd_stats(_p(x[h]), _p(dy[h]), _p(mvr[h, 0]), _p(mvr[h, 2]), _p(g32), _p(b32), _p(part[h]), M, C,
                                         int(relu), dt, st), "gf_bn_bwd_stats")
        _lib.check(L.gf_bn_pack_sums(_p(part), H, nblk, C, 0.0, _p(packed), _p(local), st), "gf_bn_pack_sums")
        _all_reduce_sum(packed)
        _lib.check(L.gf_bn_finalize_sets_bwd(_p(packed), _p(counts), H, C, _p(m12), st), "gf_bn_finalize_sets_bwd")
        for h in range(H):
            _lib.check(L.gf_bn_bwd_dx(_p(x[h]), _p(dy[h]), _p(mvr[h, 0]), _p(mvr[h, 2]), _p(g32), _p(b32), _p(m12[h, 0]),
                                      _p(m12[h, 1]), _p(dx[h]), M, C, int(relu), dt, st), "gf_bn_bwd_dx")
        dbeta, dgamma = (local[0, 0], local[0, 1]) if H == 1 else (local[:, 0].sum(0), local[:, 1].sum(0))
        if ctx.replay is not None:
            run_mean, run_var, nbt, momentum = ctx.replay
            from . import REPLAY_GATE       # the package attribute, read at call time: TrainStep rebinds it around its backward
            gate = REPLAY_GATE
            _lib.check(L.gf_bn_replay_running_n(_p(mvr), _p(counts), H, C, momentum, _p(run_mean), _p(run_var), _p(gate), st),
                       "gf_bn_replay_running_n")
            nbt.add_(H if gate is None else (gate == 0).to(nbt.dtype) * H)
        return dx, dgamma.to(gdt), dbeta.to(bdt), None, None, None, None, None, None


class _ReplayRunningStats(torch.autograd.Function):
    """Identity on y whose BACKWARD gives BatchNorm modules' running statistics one more update from the forward's batch
    statistics, group after group and set after set (the generic form of _BatchNormActSets' `replay`: single-set /
    SyncBatchNorm / torch-fallback paths, and several module calls whose replays must run in CALL order although their
    own autograd nodes run in reverse).  groups: [(bn module, [(mean, unbiased var), ...]), ...]."""

    @staticmethod
    def forward(ctx, y, groups):
        ctx.groups = [(bn, [(m.detach(), v.detach()) for m, v in stats]) for bn, stats in groups]
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        from . import REPLAY_GATE           # the package attribute, read at call time (see _BatchNormActSets.backward)
        gate = REPLAY_GATE
        with torch.no_grad():
            for bn, stats in ctx.groups:
                for mean, unbiased in stats:
                    if gate is None:
                        bn.num_batches_tracked += 1
                        mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                        bn.running_mean.mul_(1 - mom).add_(mean.to(bn.running_mean.dtype), alpha=mom)
                        bn.running_var.mul_(1 - mom).add_(unbiased.to(bn.running_var.dtype), alpha=mom)
                        continue
                    go = (gate == 0)                              # device-side: a skipped step replays nothing
                    bn.num_batches_tracked += go.to(bn.num_batches_tracked.dtype)
                    mom = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.clamp(min=1).float()
                    rm, rv = bn.running_mean, bn.running_var
                    rm.copy_(torch.where(go, rm * (1 - mom) + mean.to(rm.dtype) * mom, rm))
                    rv.copy_(torch.where(go, rv * (1 - mom) + unbiased.to(rv.dtype) * mom, rv))
        return dy, None


def replay_running_stats(y, groups):
    """y, with the replays collected in ``groups`` (``stats_out`` of batch_norm_act_sets) attached to its backward."""
    return _ReplayRunningStats.apply(y, groups) if groups else y


def _is_sync(bn):
    """True when ``bn`` exchanges its statistics across ranks (FORCE_SYNC_BN: in a one-rank group too)."""
    import torch.distributed as dist
    from . import FORCE_SYNC_BN         # the package attribute, read at call time: TrainStep(force_distributed=True) sets it
    return (isinstance(bn, torch.nn.SyncBatchNorm) and dist.is_available() and dist.is_initialized()
            and (dist.get_world_size() > 1 or FORCE_SYNC_BN))


def batch_norm_act_sets(x, bn, relu=True, replay=False, stats_out=None):
    """x [H,M,C]: ``batch_norm_act`` applied to each of the H sets in turn (set h sees the running statistics already
    updated by set h-1, exactly like H consecutive module calls), as ONE autograd node where that is possible.
    ``replay``: the backward repeats the H running-statistics updates (see _BatchNormActSets.forward); with ``stats_out`` (a
    list) the replay is NOT attached here: (bn, [(mean, unbiased var) per set]) is appended for replay_running_stats, which
    lets a caller replay several calls in call order from one node."""
    assert x.dim() == 3
    if not x.is_contiguous():
        x = x.contiguous()
    sync = _is_sync(bn)
    want = (replay or stats_out is not None) and bn.training and bn.track_running_stats and torch.is_grad_enabled() and x.requires_grad
    if (bn.training and bn.track_running_stats and bn.momentum is not None
            and bn.running_mean.dtype == torch.float32 and bn.running_mean.is_contiguous()
            and bn.running_var.is_contiguous()):
        in_node = want and stats_out is None
        if sync:        # one all-reduce per direction for the H sets, fused finalize kernels kept
            y, mvr, counts = _BatchNormActSetsSync.apply(x, bn.weight, bn.bias, bn.eps, relu, bn.running_mean, bn.running_var,
                                                         float(bn.momentum), bn.num_batches_tracked if in_node else None)
        else:
            y, mvr = _BatchNormActSets.apply(x, bn.weight, bn.bias, bn.eps, relu, bn.running_mean, bn.running_var,
                                             float(bn.momentum), bn.num_batches_tracked if in_node else None)
            counts = None
        with torch.no_grad():
            bn.num_batches_tracked += x.shape[0]
        if want and stats_out is not None:
            if counts is None:
                unb = [x.shape[1] / max(x.shape[1] - 1.0, 1.0)] * x.shape[0]
            else:
                unb = [counts[h] / (counts[h] - 1.0).clamp(min=1.0) for h in range(x.shape[0])]
            stats_out.append((bn, [(mvr[h, 0], mvr[h, 1] * unb[h]) for h in range(x.shape[0])]))
        return y
    stats = [] if want else None
    y = torch.stack([batch_norm_act(x[h], bn, relu, stats_out=stats) for h in range(x.shape[0])])
    if not stats:
        return y
    if stats_out is not None:
        stats_out.append((bn, stats))
        return y
    return _ReplayRunningStats.apply(y, [(bn, stats)])        # (one node: the sets replay in call order)


def batch_norm_act(x, bn, relu=True, replay=False, stats_out=None):
    """x [M,C] channels-last through ``bn`` (an nn.BatchNorm1d / SyncBatchNorm that owns the affine
    parameters and running statistics), then ReLU when ``relu``.  Training mode uses batch statistics
    (summed across ranks when ``bn`` was converted to SyncBatchNorm) and updates the running
    statistics like torch (momentum, unbiased variance, num_batches_tracked); eval uses them.
    ``replay``: the backward repeats that update (the module sits inside an activation-checkpointed block of the
    reference: see _BatchNormActSets.forward); ``stats_out``: a list that receives this call's (mean, unbiased var)
    instead (batch_norm_act_sets replays several calls in order from one node)."""
    assert x.dim() == 2
    if not x.is_contiguous():
        x = x.contiguous()
    if bn.training or not bn.track_running_stats:
        sync = _is_sync(bn)
        track = bn.training and bn.track_running_stats
        fused_running = (track and not sync and bn.momentum is not None and bn.running_mean.dtype == torch.float32
                         and bn.running_mean.is_contiguous() and bn.running_var.is_contiguous())
        replay = replay and track and torch.is_grad_enabled() and x.requires_grad
        if fused_running:       # the finalize kernel updates the running statistics in place
            y, mean, var, _ = _BatchNormAct.apply(x, bn.weight, bn.bias, None, None, bn.eps, True, relu, sync,
                                                  bn.running_mean, bn.running_var, float(bn.momentum))
            with torch.no_grad():
                bn.num_batches_tracked += 1
            if replay or stats_out is not None:
                stat = (mean, var * (x.shape[0] / max(x.shape[0] - 1.0, 1.0)))
                if stats_out is not None:
                    stats_out.append(stat)
                else:
                    y = _ReplayRunningStats.apply(y, [(bn, [stat])])
            return y
        y, mean, var, n_t = _BatchNormAct.apply(x, bn.weight, bn.bias, None, None, bn.eps, True, relu, sync)
        if track:
            with torch.no_grad():
                if not torch.is_tensor(n_t) or n_t.numel() == 0:
                    n_t = torch.full((), float(x.shape[0]), dtype=torch.float32, device=x.device)
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                unbiased = var * (n_t / (n_t - 1).clamp(min=1.0))
                bn.running_mean.mul_(1 - mom).add_(mean.to(bn.running_mean.dtype), alpha=mom)
                bn.running_var.mul_(1 - mom).add_(unbiased.to(bn.running_var.dtype), alpha=mom)
            if stats_out is not None:
                stats_out.append((mean, unbiased))
            elif replay:
                y = _ReplayRunningStats.apply(y, [(bn, [(mean, unbiased)])])
        return y
    rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
    return _BatchNormAct.apply(x, bn.weight, bn.bias, bn.running_mean, rstd, bn.eps, False, relu, False)[0]
