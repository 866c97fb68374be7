"""Line "extractor" for segments that arrive with the view (a dataset worker, a feature cache).

The reference's line detector (gluefactory/models/lines/lsd.py) is third-party CPU code; what it does AFTER the detector
(:28-53) is all a downstream stage depends on, and that part is restated here in batched torch ops on whatever device the
segments live on:

  * segments shorter than ``min_length`` are dropped (``>=`` keeps a segment of exactly that length),
  * the ``max_num_lines`` best by score are kept, in descending score order (ties: the earlier segment first),
  * under ``force_num_lines`` every image is padded to ``max_num_lines`` with zero segments, score 0, valid False.

``{"lines" [B,M,2,2], "line_scores" [B,M], optional "valid_lines" [B,M]} -> {"lines", "line_scores", "valid_lines"}``.
Input segments with ``valid_lines`` False count as absent.  Without ``force_num_lines`` the number of lines is data
dependent (one host read) and, as in the reference, only a batch whose images keep the same number can be stacked.
The score is taken as given: LSD's ``nfa * sqrt(length)`` is the producer's business.
"""
import torch

from ..base_model import BaseModel


class GivenLines(BaseModel):
    default_conf = {
        "min_length": 15,
        "max_num_lines": None,
        "force_num_lines": False,
    }
    required_data_keys = ["lines", "line_scores"]
    batchable_views = True

    def _init(self, conf):
        if conf.force_num_lines:
            assert conf.max_num_lines is not None, "Missing max_num_lines parameter"

    def _forward(self, data):
        lines, scores = data["lines"].float(), data["line_scores"].float()
        b, m = scores.shape
        d = lines[:, :, 1] - lines[:, :, 0]
        keep = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) >= self.conf.min_length
        if data.get("valid_lines") is not None:
            keep = keep & data["valid_lines"].bool()
        # kept segments by descending score, the dropped ones behind them (stable: ties keep their order)
        key = torch.where(keep, scores, scores.new_full((), float("-inf")))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        k = m if self.conf.max_num_lines is None else min(m, int(self.conf.max_num_lines))
        order = order[:, :k]
        valid = keep.gather(1, order)
        lines = lines.gather(1, order[:, :, None, None].expand(b, k, 2, 2))
        scores = scores.gather(1, order)
        if self.conf.force_num_lines:
            pad = int(self.conf.max_num_lines) - k
            lines = torch.where(valid[:, :, None, None], lines, torch.zeros_like(lines))
            scores = torch.where(valid, scores, torch.zeros_like(scores))
            if pad > 0:
                lines = torch.cat([lines, lines.new_zeros(b, pad, 2, 2)], 1)
                scores = torch.cat([scores, scores.new_zeros(b, pad)], 1)
                valid = torch.cat([valid, valid.new_zeros(b, pad)], 1)
        else:
            counts = valid.sum(1).tolist()                       # the host read of a data-dependent shape
            if len(set(counts)) > 1:
                raise ValueError("images keep different numbers of lines: set force_num_lines")
            n = counts[0] if counts else 0
            lines, scores, valid = lines[:, :n], scores[:, :n], valid[:, :n]
        return {"lines": lines, "line_scores": scores, "valid_lines": valid}

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = GivenLines
