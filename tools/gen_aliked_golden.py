"""Writes tests/golden/aliked.npz: inputs and the outputs of the UNMODIFIED reference ALIKED module
(gluefactory/models/extractors/aliked.py, imported through the torchvision stand-in of tests/aliked_stubs) for two cases
of tests/aliked_cases.py.  No weights are stored: tests rebuild them from the seed (aliked_cases.build_model).

    python tools/gen_aliked_golden.py /path/to/glue-factory
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import aliked_cases as ac  # noqa: E402


def main(ref):
    def no_network(*a, **k):
        raise RuntimeError("the reference module tried to download weights")
    torch.hub.load_state_dict_from_url = no_network
    paths = ac.reference_paths(ref)
    sys.path[:0] = paths[:-1]
    sys.path.append(paths[-1])
    from gluefactory.models.extractors.aliked import ALIKED as RefALIKED
    out = {}
    for name in ac.GOLDEN_CASES:
        conf, data = ac.sweep_case(name)
        model = RefALIKED({**conf, "pretrained": False}).eval()
        model.load_state_dict(ac.build_model(conf).state_dict(), strict=True)
        with torch.no_grad():
            pred = model({k: v.clone() for k, v in data.items()})
        for k, v in data.items():
            out[f"{name}.data.{k}"] = v.numpy()
        for k, v in pred.items():
            out[f"{name}.pred.{k}"] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "aliked.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
