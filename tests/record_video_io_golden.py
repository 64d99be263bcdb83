#!/usr/bin/env python3
"""Record tests/golden/video_io_ref.npz: inputs and what the reference's own statements (fast_infer.py:88-90, the loader's
float conversion; videox_fun/utils/utils.py:60-67, the writer's byte conversion) make of them.  Needs the reference tree
(oracle/ref_import.py: VIDEOCOF_REFERENCE); the statements are read from it and executed, none of them is restated here.

    python tests/record_video_io_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_video_io_host as H  # noqa: E402


def main():
    assert H.reference_present(), f"no reference tree at {H.REFERENCE_ROOT}"
    g = torch.Generator().manual_seed(2024)
    frames = torch.randint(0, 256, (3, 18, 28, 3), generator=g, dtype=torch.uint8)
    frames.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)                  # every byte value
    video_bf16 = torch.randn(1, 3, 3, 18, 28, generator=g).mul(0.6).bfloat16()
    video_f32 = torch.randn(1, 3, 3, 18, 28, generator=g).mul(0.6)

    def writer(video):
        return H.run_reference_writer((video / 2 + 0.5).clamp(0, 1).cpu().float())          # pipeline_wan.py:426-427, then the writer

    out = dict(frames_u8=frames.numpy(), loader_out=H.run_reference_loader(frames.numpy()).numpy(),
               writer_out_boundary=writer(H.boundary_video()),
               video_bf16_bits=video_bf16.view(torch.int16).numpy(), writer_out_bf16=writer(video_bf16),
               video_f32=video_f32.numpy(), writer_out_f32=writer(video_f32))
    path = H.FIXTURE
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
