#!/usr/bin/env python3
"""Record tests/golden/video_compose_ref.npz: inputs and what the reference's own statements (fast_infer.py:183-204,
``_normalize_to_01`` and the body of ``save_side_by_side``; fast_infer.py:88-90, the loader's float conversion;
videox_fun/utils/utils.py:60-67, the writer) make of them.  Needs the reference tree (oracle/ref_import.py: VIDEOCOF_REFERENCE);
the statements are read from it and executed, none of them is restated here (``make_grid``: see test_frame_compose_host.py).

    python tests/record_video_compose_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_frame_compose_host as H  # noqa: E402


def main():
    assert H.reference_present(), "no reference tree (VIDEOCOF_REFERENCE)"
    x = H.inputs()
    out = {"in_" + k: v.numpy() for k, v in x.items()}
    out.update(H.reference_outputs(x))
    np.savez_compressed(H.FIXTURE, **out)
    print(H.FIXTURE, os.path.getsize(H.FIXTURE), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
