#!/usr/bin/env python3
"""The mix gather of a balanced WindowSet (chebgcn_gather_windows_mix) measured beside the plain gather
(chebgcn_gather_windows) for one training batch: random planes [T, Mp], B random windows, every window the mean of ``cnt``
random source windows, cnt in --cnt (smax = cnt).  Device events around single launches, the arms interleaved in --rounds
rounds of --reps launches: median / min / max us and the achieved rate on the algorithmic bytes, 4 * (cnt + 1) * B * C * Mp
(the plain gather: cnt = 1), in GB/s and as a share of 8.0 TB/s.

Prints one JSON line.  Needs a GPU; there is no CPU fallback.

    python tools/mix_gather_bench.py [--M 10242] [--C 15] [--B 64] [--T 4000] [--cnt 1,2,4] [--rounds 5] [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gcn_fmri_decoding_amd import _lib, ops   # noqa: E402
from series_bench import HBM_SPEC, event_us, spread   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, default=10242)
    ap.add_argument('--C', type=int, default=15)
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--T', type=int, default=4000)
    ap.add_argument('--cnt', default='1,2,4')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--tables', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mix_gather_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    M, C, B, T = args.M, args.C, args.B, args.T
    Mp = ops.plane_stride(M)
    rs = np.random.RandomState(1)
    planes = torch.randn((T, Mp), device=dev)
    S = 4 * B
    idx = torch.as_tensor(rs.permutation(S)[:B].astype(np.int32)).to(dev)
    out = torch.empty((B, C, Mp), dtype=torch.float32, device=dev)
    scale = shift = None
    if args.tables:
        scale, shift = torch.rand((C, Mp), device=dev) + 0.5, torch.randn((C, Mp), device=dev)
    rows1 = torch.as_tensor(rs.randint(0, T - C + 1, size=S).astype(np.int64)).to(dev)
    arms = {'gather_windows': (1, lambda: ops.gather_windows(planes, rows1, M, C, idx, scale, shift, out))}
    for n in [int(v) for v in args.cnt.split(',')]:
        rows = torch.as_tensor(rs.randint(0, T - C + 1, size=(S, n)).astype(np.int64)).to(dev)
        cnt = torch.full((S,), n, dtype=torch.int32, device=dev)
        arms['gather_windows_mix cnt=%d' % n] = (n, lambda rows=rows, cnt=cnt: ops.gather_windows_mix(
            planes, rows, cnt, M, C, idx, scale, shift, out))
    us, kernel = {k: [] for k in arms}, {}
    for k, (_, fn) in arms.items():
        event_us(fn, 5)
        kernel[k] = _lib.last_dispatch()
    for _ in range(args.rounds):
        for k, (_, fn) in arms.items():
            us[k] += event_us(fn, args.reps)
    res = {'device': torch.cuda.get_device_name(0), 'M': M, 'Mp': Mp, 'C': C, 'B': B, 'T': T, 'tables': bool(args.tables),
           'rounds': args.rounds, 'reps': args.reps, 'arms': {}}
    for k, (n, _) in arms.items():
        nbytes = 4.0 * (n + 1) * B * C * Mp
        med = float(np.median(us[k]))
        res['arms'][k] = dict(spread(us[k]), kernel=kernel[k], bytes=nbytes, GBs=nbytes / (med * 1e-6) / 1e9,
                              share_of_8TBs=nbytes / (med * 1e-6) / HBM_SPEC)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
