"""torch.autograd.Function wrappers around the HIP launchers of libgf_amd.so.

PyTorch is plumbing here (device memory, streams, autograd graph); every op below calls the
C ABI of include/gf_amd.h through ctypes with raw device pointers and the current HIP stream.
There is no CPU or eager fallback: a non-CUDA tensor or a missing library raises.

One sub-module per kernel family of csrc/; callers use the names re-exported here (``ops.linear(...)``).

Process-global state, each piece with one home:
* mutable containers live in the module that fills them, are re-exported by identity and are only mutated in place:
  _LP_CACHE / _LP_PTR / _LP_T / _LP_FLAT (_params), LIBRARY_GEMMS (_linear), _SPARSE_SUMS (_nll), COLLECTIVES (_batchnorm);
* the four rebindable scalars XBWD_ENABLED, FOLD_ENABLED, REPLAY_GATE and FORCE_SYNC_BN are attributes of THIS package and of
  nothing else: writers assign ``ops.NAME = value``, and the consumer of each reads it from the package when it is called
  (a copy imported into a sub-module would not see the assignment).
"""
from ._base import BF16, F32, _chk, _dt, _p, _s3, _stream
from ._attention import (ATTN_SPLIT, LN2, SharedGradSum, attention, attention_qkv, attn_bwd_raw, attn_fwd_raw, attn_premul,
                         cross_attention, cross_attention_stacked, self_attention_rotary)
from ._params import (_LP_CACHE, _LP_FLAT, _LP_PTR, _LP_T, _DerivedWeight, _lp, _wt_t, derived_weight, folded_linear,
                      invalidate_precast, precast)
from ._linear import (LIBRARY_GEMMS, GradChain, colsum, gemm, gemm_takes, linear, linear_cat, ln_gelu, rowdot, rowdot2,
                      small_linear)
from ._nll import _SPARSE_SUMS, _known_sums, nll_positive_terms, nll_terms
from ._assignment import (_head_bwd, assign_write, bgemm, dual_lse, dual_lse_stacked, filter_matches, lg_layer_loss,
                          n_pair_loss, nn_filter, rows_argmax, rows_lse, rows_top2, similarity)
from ._sinkhorn import sinkhorn, sinkhorn_schedule
from ._batchnorm import (COLLECTIVES, _BatchNormActSetsSync, _ReplayRunningStats, batch_norm_act, batch_norm_act_sets,
                         replay_running_stats)
from ._lines import (_line_graph_sorted, dense_log_double_softmax, line_aggregate, line_gather, line_graph, line_pair_scores,
                     rows_gather)

XBWD_ENABLED = True      # tools/probe/ab_matcher.py --switch XBWD_ENABLED: same-process A/B against two gf_attn_bwd_acc calls
                         # (read by _CrossAttentionStacked.backward)

FOLD_ENABLED = True      # tools/probe/ab_matcher.py switches it off for a same-process A/B of the folded blocks (read by folded_linear)

# The reference `continue`s BEFORE its backward when the loss is non-finite or not differentiable (train.py:477-488): the
# activation-checkpointed blocks are then not re-run and their BatchNorm statistics take ONE update.  TrainStep always runs its
# backward (the gradient reducer needs every rank's), so it parks its device-side "bad" flag here for the duration of the
# backward and the replays of _batchnorm become no-ops on such a step (fp32 scalar tensor, non-zero = skip; None = always replay).
REPLAY_GATE = None

FORCE_SYNC_BN = False     # tests: take the SyncBatchNorm exchange in a one-rank group too (TrainStep(force_distributed=True))

# data-preparation kernels (csrc/hviews.hip): not autograd ops; their wrappers live with the stage that uses them
from ..data._views_ops import filter_views, warp_views  # noqa: E402
