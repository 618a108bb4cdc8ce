#!/usr/bin/env python
"""Host cost of the checked Python face: the ten library calls of one FramePairPipeline step (stereo() + track(), every
output preallocated) on host tensors, with a `_call` that does nothing -- what device.py itself spends per step on checks,
records and pointer lists, with no device and no library.

    python scripts/time_context_calls.py [--root TREE] [--steps 3000]

prints one JSON line {"median_us_per_step": ..., "min_us_per_step": ...}.  --root: the checkout whose package is timed (this
one by default); compare two trees in alternating fresh processes."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=3000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from vo_single_camera_sos_amd import _lib
    from vo_single_camera_sos_amd.device import Context
    from vo_single_camera_sos_amd.pipeline import FramePairPipeline, RigConfig

    torch.Tensor.is_cuda = property(lambda self: True)      # host tensors pass the residency rule
    ctx = Context.__new__(Context)
    ctx.device, ctx._h = torch.device("cpu"), None
    ctx._lib = SimpleNamespace(**{name: name for name in _lib.SIGNATURES})
    ctx._call = lambda fn, *a: None
    geo = (1200, 300, 0.5, 3.0)
    rig = RigConfig(pano_top=geo, pano_bot=geo, F_top=(0, 0, 1.0), F_bot=(0, 0, -1.0), min_range=0.5, max_range=70.0,
                    f2f_max_hdiff=75.0)
    pipe = FramePairPipeline(ctx, rig, 2, nmask=3, bucket_cap=8, frame_cap=16, max_iter=10)
    times = []
    for i in range(args.steps + 200):
        t0 = time.perf_counter_ns()
        pipe.stereo()
        pipe.track()
        times.append((time.perf_counter_ns() - t0) / 1e3)
    times = times[200:]
    print(json.dumps({"median_us_per_step": round(statistics.median(times), 2), "min_us_per_step": round(min(times), 2)}))


if __name__ == "__main__":
    main()
