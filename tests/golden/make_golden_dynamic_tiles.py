"""Golden fixture of the register engines' outputs before their workgroups took their work from a counter: dynamic_tiles.npz.

NEEDS AN MI355X AND THE BUILD TO RECORD (the commit in front of the dynamic tile queue): it runs fixture_outputs() of
tests/test_gpu_dynamic_tiles.py -- the x2 / bf16x3 synthesis images and the f16x2 (with refinement) / f16x3 fused renders of that
file's cases -- and stores one SHA-256 per batch item and array (uint8 [B, 32]); data only.
Run:  python tests/golden/make_golden_dynamic_tiles.py [output path]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import conftest  # noqa: E402,F401  (puts the repository and the oracle on sys.path)
import test_gpu_dynamic_tiles as T  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    out = T.fixture_outputs()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
