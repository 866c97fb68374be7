"""Writes tests/golden/wireframe.npz: inputs and the REFERENCE's outputs of three wireframe scenes.

Runs where the reference checkout is present (python tools/gen_wireframe_golden.py [reference root]).  The unmodified
``gluefactory.models.lines.wireframe`` is imported in place (with the omegaconf stand-in of oracle/stubs); a subclass
overrides only ``_init``, to plug in two tiny deterministic sub-extractors that hand back the scene's tensors.  Scenes
(tests/wireframe_cases.py): 128 x 160 image, s = 8, C = 64, N = 64 keypoints, L = 24 lines of which 6 are zero padding --
forced mode with both merges, forced mode with ``merge_line_endpoints: false``, and the batch-of-one variable-count mode.
The file holds arrays only: ``<scene>.in.<key>`` the inputs, ``<scene>.out.<key>`` the reference's outputs, and
``<scene>.suppressed`` the keypoints the reference replaced or removed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "stubs")]
sys.path.append(REF)

import wireframe_cases as wc  # noqa: E402
from gluefactory.models.lines.wireframe import WireframeExtractor as RefWireframe  # noqa: E402

CONFS = {
    "forced": dict(force=True, merge_line_endpoints=True),
    "forced_nomerge": dict(force=True, merge_line_endpoints=False),
    "variable": dict(force=False, merge_line_endpoints=True),
}


class Feed(torch.nn.Module):
    """A sub-extractor that returns copies of the scene's tensors."""

    def __init__(self, tensors):
        super().__init__()
        self.tensors = tensors

    def forward(self, data):
        return {k: v.clone() for k, v in self.tensors.items()}


def reference_outputs(scene, force, merge_line_endpoints):
    t = {k: torch.from_numpy(v) for k, v in scene.items()}

    class Fixture(RefWireframe):
        def _init(self, conf):
            self.point_extractor = Feed({k: t[k] for k in ("keypoints", "keypoint_scores", "descriptors", "dense_descriptors")})
            self.line_extractor = Feed({k: t[k] for k in ("lines", "line_scores", "valid_lines")})

    n_lines, n_kpts = t["lines"].shape[1], t["keypoints"].shape[1]
    model = Fixture({
        "point_extractor": {"name": "fixture", "max_num_keypoints": n_kpts, "force_num_keypoints": force},
        "line_extractor": {"name": "fixture", "max_num_lines": n_lines, "force_num_lines": force},
        "wireframe_params": {"merge_points": True, "merge_line_endpoints": merge_line_endpoints, "nms_radius": 3},
    })
    h, w = wc.GOLDEN_GEOMETRY["hw"]
    torch.manual_seed(0)
    with torch.no_grad():
        return model({"image": torch.zeros(t["lines"].shape[0], 1, h, w)})


def main():
    out = {}
    for name, conf in CONFS.items():
        scene = wc.golden_inputs(name)
        assert wc.band_violations(scene["lines"], scene["keypoints"], 3, 3) == 0
        pred = reference_outputs(scene, **conf)
        for k, v in scene.items():
            out[f"{name}.in.{k}"] = v
        for k, v in pred.items():
            out[f"{name}.out.{k}"] = v.numpy()
        ends = torch.from_numpy(scene["lines"]).reshape(scene["lines"].shape[0], -1, 2)
        dist = torch.norm(torch.from_numpy(scene["keypoints"])[:, :, None] - ends[:, None], dim=-1)
        out[f"{name}.suppressed"] = (dist < 3).any(2).numpy()
    path = os.path.join(ROOT, "tests", "golden", "wireframe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: tuple(v.shape) for k, v in out.items() if ".out." in k and k.startswith("forced.")})


if __name__ == "__main__":
    main()
