"""Time sosvo_detect_gft on a problem with more candidates than its selection sorts: white noise 480 x 640 (20 285
candidates at quality 1e-4) at cap 512 (4096 candidates kept; the 2048 first pass hands over) and cap 2048 (16384 kept).
Prints one JSON line per capacity: the median and the spread of the GPU time per call from stream events.  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_gft_overflow.py` for the per-kernel times (the selection
kernels are gft_select_kernel<2048, 512> + <4096, 512> for cap 512 and gft_select_kernel<16384, 1024> for cap 2048)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vo_single_camera_sos_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    ctx = Context(0)
    img = torch.from_numpy(np.random.default_rng(77).integers(0, 256, (1, 480, 640), dtype=np.uint8)).to(ctx.device)
    bits = torch.ones((1, 480, 640), dtype=torch.uint32, device=ctx.device)
    for cap in (512, 2048):
        kp = torch.zeros((1, cap, 2), dtype=torch.float32, device=ctx.device)
        n = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
        status = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
        call = lambda: ctx.detect_gft(img, bits, 1, 1, cap, quality=1e-4, min_distance=5.0, max_corners=0, kp=kp, n=n, status=status)  # noqa: E731
        for _ in range(args.warmup):
            call()
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.sort(ms)
        print(json.dumps(dict(cap=cap, n=int(n.item()), status=int(status.item()), reps=args.reps, ms_median=float(np.median(ms)),
                              ms_min=float(ms[0]), ms_max=float(ms[-1]))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
