"""Nearest-neighbour matcher for L2-normalised descriptors: mutual check, ratio and distance thresholds, N-pair loss.

Plugin-surface mirror of gluefactory/models/matchers/nearest_neighbor_matcher.py:15-97 -- same configuration keys
(``ratio_thresh``, ``distance_thresh``, ``mutual_check``, ``loss``), same required inputs, same output names and dtypes,
same ``temperature`` parameter when ``loss: N_pair``.

The reference builds the [B,M,N] similarity, takes ``topk(2)`` of it in both directions and gathers through the result.
Here the matches never need that tensor: ``ops.rows_top2`` streams one descriptor set past the other on the matrix cores
and keeps (best, arg, second) per row, and ``ops.nn_filter`` applies find_nn's thresholds and mutual_check to the two
triples.  ``similarity`` (one batched product, an autograd node whose backward is two more) and ``log_assignment``
(``dual_lse`` + ``assign_write`` with zero bins: 2 sim - lse_row - lse_col, never re-reading ``similarity``) are the dense
outputs the reference also returns; ``dense_outputs: False`` (ours) skips both for evaluation at large N.

The N-pair loss (reference lines 76-93) runs as dense HIP passes over ``pred["similarity"]`` with the positives of
``gt_assignment`` as a sparse list (``gt_assignment_col0`` when the ground-truth producer supplied it: no scan, no host
synchronisation).  Two checks of the reference are left out because each forces a host synchronisation per step: the
``torch.any(sim > 1 + 1e-6)`` warning (line 78) and the NaN assert (line 82).

One positive per row with ``gt_assignment_col0``: when the batch carries that key the loss reads it ALONE, so at most one
positive of each row of ``gt_assignment`` reaches the loss (the convention of LightGlue._gt_sparse; every ground-truth
producer of this package writes a one-to-one assignment, where the two agree).  The reference sums over every true entry
of ``gt_assignment``; a many-to-one ground truth gives its loss only without ``gt_assignment_col0`` in the batch.
"""
import torch

from .. import ops
from ..base_model import BaseModel
from ..metrics import matcher_metrics


class NearestNeighborMatcher(BaseModel):
    default_conf = {
        "ratio_thresh": None,
        "distance_thresh": None,
        "mutual_check": True,
        "loss": None,
        "dense_outputs": True,     # ours: False skips `similarity` and `log_assignment` ([B,M,N] and [B,M+1,N+1] fp32)
    }
    required_data_keys = ["descriptors0", "descriptors1"]

    def _init(self, conf):
        if conf.loss == "N_pair":
            if not conf.dense_outputs:
                raise ValueError("nearest_neighbor_matcher: loss N_pair reads pred['similarity'], which "
                                 "dense_outputs: False does not produce")
            self.register_parameter("temperature", torch.nn.Parameter(torch.tensor(1.0)))

    def _compute_dtype(self, desc0, desc1):
        if torch.is_autocast_enabled() or (desc0.dtype == torch.bfloat16 and desc1.dtype == torch.bfloat16):
            return torch.bfloat16
        return torch.float32

    @torch.compiler.disable
    def forward(self, data):
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        desc0, desc1 = data["descriptors0"], data["descriptors1"]
        if not (desc0.is_cuda and desc1.is_cuda):
            raise RuntimeError("glue_factory_amd.NearestNeighborMatcher runs on the MI355X HIP path only "
                               "(move the batch to the GPU; there is no CPU fallback)")
        T = self._compute_dtype(desc0, desc1)  # read the autocast state before switching it off
        with torch.autocast(device_type="cuda", enabled=False):
            return self._forward(desc0.to(T), desc1.to(T))

    def _forward(self, desc0, desc1):
        conf = self.conf
        b, m, _ = desc0.shape
        n = desc1.shape[1]
        dev = desc0.device
        if conf.ratio_thresh and min(m, n) < 2:
            raise ValueError(f"nearest_neighbor_matcher: ratio_thresh needs two candidates per keypoint, got {m} x {n}")
        if m == 0 or n == 0:       # nothing to launch: nobody is matched
            pred = {"matches0": torch.full((b, m), -1, dtype=torch.int64, device=dev),
                    "matches1": torch.full((b, n), -1, dtype=torch.int64, device=dev),
                    "matching_scores0": torch.zeros((b, m), dtype=torch.float32, device=dev),
                    "matching_scores1": torch.zeros((b, n), dtype=torch.float32, device=dev)}
            if conf.dense_outputs:
                pred["similarity"] = desc0.new_zeros((b, m, n))
                pred["log_assignment"] = torch.zeros((b, m + 1, n + 1), dtype=torch.float32, device=dev)
            return pred
        m0, m1, s0, s1 = ops.nn_filter(ops.rows_top2(desc0, desc1), ops.rows_top2(desc1, desc0),
                                       conf.ratio_thresh, conf.distance_thresh, conf.mutual_check)
        pred = {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1}
        if conf.dense_outputs:
            pred["similarity"] = ops.similarity(desc0, desc1)
            r, c = ops.dual_lse(desc0, desc1)
            zm, zn = r.new_zeros((b, m)), r.new_zeros((b, n))
            pred["log_assignment"] = ops.assign_write(desc0, desc1, -r, -c, zm, zn, alpha=2.0, corner=0.0)
        return pred

    @staticmethod
    def _positives(data):
        """(b, i, j) index vectors of the positives of gt_assignment; from ``gt_assignment_col0`` (the single positive
        column of each row, -1 if none) a fixed-length list with j = -1 as padding, as LightGlue._gt_sparse builds it."""
        col0 = data.get("gt_assignment_col0")
        if col0 is None:
            return data["gt_assignment"].nonzero(as_tuple=True)                        # one host read per step
        bsz, m = col0.shape
        dev = col0.device
        return (torch.arange(bsz, device=dev).repeat_interleave(m), torch.arange(m, device=dev).repeat(bsz),
                col0.reshape(-1).long())

    @torch.compiler.disable
    def loss(self, pred, data):
        if self.conf.loss != "N_pair":
            raise NotImplementedError
        if "similarity" not in pred:
            raise ValueError("nearest_neighbor_matcher: loss N_pair reads pred['similarity'] (dense_outputs: True)")
        with torch.autocast(device_type="cuda", enabled=False):
            nll, num = ops.n_pair_loss(pred["similarity"], self.temperature, self._positives(data))
            losses = {"n_pair_nll": nll, "total": nll, "num_matchable": num,
                      "n_pair_temperature": self.temperature[None]}
            metrics = {} if self.training else matcher_metrics(pred, data)
        return losses, metrics


__main_model__ = NearestNeighborMatcher
