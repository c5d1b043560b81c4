#!/usr/bin/env python3
"""Training on scans (cgcnn.stage_windows / fit_series) measured, at the two shapes of tools/saliency_bench.py (atlas: 360
vertices, batch 128; config1: BASELINE configs[1], M = 10466, batch 64; both channel 15):

  gather    chebgcn_gather_windows against chebgcn_perm_data for one training batch, device events around single launches,
            the two interleaved in --rounds rounds of --reps launches: median / min / max us and the share of the HBM roofline
            (algorithmic bytes 2 * B * C * Mp * 4 over 8.0 TB/s spec and over the 6.29 TB/s a float4 copy reaches);
  step      the training step (gather into the step's input + train_step) from a WindowSet against the step from the staged
            [S, M, C] array -- the array arm is the code path of the commit before this feature, unchanged -- same model, same
            process, alternating, --rounds rounds of --steps synchronised steps each: ms per step per round;
  stats     WindowSet.fit_scaler() (chebgcn_window_stats, its three launches, device-synchronised) for a training set of
            --runs runs of --T time points at stride 1;
  memory    device bytes of the WindowSet against the materialised array at stride 1;
  events    chebgcn_gather_windows_indexed (windows as lists of rows: events.match_events, fit_events) beside
            chebgcn_gather_windows on the SAME contiguous windows at fold = 1 without sources, then with fold = 2 and with
            cnt = 4 sources per window, interleaved like the gather leg (bytes: (fold * cnt + 1) * B * C * Mp * 4), and
            chebgcn_window_stats_indexed beside chebgcn_window_stats on those windows.

Prints one JSON line.  Needs a GPU; there is no CPU fallback.

    python tools/series_bench.py [--shapes atlas,config1] [--rounds 5] [--reps 50] [--steps 30] [--runs 8] [--T 500] [--legs gather,step,stats,events] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gcn_fmri_decoding_amd import ops   # noqa: E402
from saliency_bench import build   # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def event_us(fn, reps):
    """Device microseconds of ``reps`` single launches of fn(), one event pair each."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        out.append((a, b))
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in out]


def spread(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='atlas,config1')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=8)
    ap.add_argument('--T', type=int, default=500)
    ap.add_argument('--legs', default='gather,step,stats,events')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('series_bench: no GPU visible (the measurement does not fall back to the CPU)')
    dev = torch.device('cuda', 0)
    legs = set(args.legs.split(','))
    res = {'device': torch.cuda.get_device_name(0), 'cus': torch.cuda.get_device_properties(0).multi_processor_count,
           'torch': torch.__version__, 'hip': torch.version.hip, 'rounds': args.rounds, 'reps': args.reps, 'steps': args.steps}
    for shape in args.shapes.split(','):
        net, B = build(shape, dev)
        net.dropout = 1
        C, M = int(net.channel), int(net._M0)
        Mp = ops.plane_stride(M)
        rs = np.random.RandomState(1)
        runs = [rs.randn(args.T, M).astype(np.float32) for _ in range(args.runs)]
        ws = net.stage_windows(runs)                                    # every window, stride 1
        S = len(ws)
        x = net.stage(ws.materialise())
        labels = torch.as_tensor(rs.randint(0, int(net.M[-1]), S)).to(dev)
        r = {'M': M, 'Mp': Mp, 'batch': B, 'channel': C, 'T_total': args.runs * args.T, 'windows': S}
        r['memory'] = {'window_set_MB': ws.nbytes / 2 ** 20, 'array_MB': x.numel() * 4 / 2 ** 20,
                       'ratio': x.numel() * 4 / ws.nbytes}

        # ---- the two gathers, one batch
        idx = torch.as_tensor(rs.permutation(S)[:B].astype(np.int32)).to(dev)
        out = ops.plane_empty(B, C, M, dev)
        nbytes = 2.0 * B * C * Mp * 4
        arms = {'gather_windows': lambda: net._gather(ws, idx, out=out), 'perm_data': lambda: net._gather(x, idx, out=out)}

        def interleaved(arms):
            us = {k: [] for k in arms}
            for fn in arms.values():
                event_us(fn, 5)
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    us[k] += event_us(fn, args.reps)
            return us
        if 'gather' in legs:
            r['gather'] = {k: dict(spread(v), bytes=nbytes, share_of_8TBs=nbytes / (np.median(v) * 1e-6) / HBM_SPEC,
                                   share_of_copy_rate=nbytes / (np.median(v) * 1e-6) / HBM_COPY)
                           for k, v in interleaved(arms).items()}

        # ---- the training step from either dataset, alternating
        if 'step' in legs:
            def steps(data, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    b0 = (i * B) % (S - B)
                    sel = order[b0:b0 + B]
                    net.train_step(net._gather(data, sel, out=net.step_inputs()[0]), labels[sel.long()])
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / n
            order = torch.as_tensor(rs.permutation(S).astype(np.int32)).to(dev)
            if net._auto_step_graph():
                net.enable_step_graph(True)
            for data in (ws, x):
                steps(data, 6)                                              # warm-up (and the capture, on the atlas shape)
            ms = {'window_set': [], 'array': []}
            for _ in range(args.rounds):
                ms['window_set'].append(steps(ws, args.steps))
                ms['array'].append(steps(x, args.steps))
            r['step_ms'] = {k: dict(spread(v), rounds=v) for k, v in ms.items()}
            r['step_ms']['window_set_over_array'] = float(np.median(ms['window_set']) / np.median(ms['array']))
            r['step_ms']['captured'] = net._sg is not None

        # ---- the scaler's statistics
        if 'stats' in legs:
            def fit_scaler():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.window_stats(ws.planes, ws.rows, M, C)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)
            fit_scaler()
            t = [fit_scaler() for _ in range(max(5, args.rounds))]
            series_bytes = 4.0 * args.runs * args.T * Mp
            r['window_stats_ms'] = dict(spread(t), series_MB=series_bytes / 2 ** 20,
                                        series_bytes_over_median_TBs=series_bytes / (np.median(t) * 1e-3) / 1e12)
        # ---- windows as lists of rows beside the contiguous gather, on the same windows
        if 'events' in legs:
            idx1 = (ws.rows[:, None] + torch.arange(C, device=dev)[None, :]).contiguous()
            idx2 = torch.cat([idx1, idx1[torch.as_tensor(rs.permutation(S)).to(dev)]], dim=1).contiguous()      # fold = 2
            src = torch.as_tensor(rs.randint(0, S, size=(S, 4)).astype(np.int64)).to(dev)
            cnt = torch.full((S,), 4, dtype=torch.int32, device=dev)
            ev_arms = {
                'gather_windows': (1, lambda: ops.gather_windows(ws.planes, ws.rows, M, C, idx, None, None, out)),
                'indexed fold=1': (1, lambda: ops.gather_windows_indexed(ws.planes, idx1, M, C, 1, sample=idx, out=out)),
                'indexed fold=2': (2, lambda: ops.gather_windows_indexed(ws.planes, idx2, M, C, 2, sample=idx, out=out)),
                'indexed fold=1 cnt=4': (4, lambda: ops.gather_windows_indexed(ws.planes, idx1, M, C, 1, src, cnt, idx, out=out)),
            }
            us = interleaved({k: fn for k, (_, fn) in ev_arms.items()})
            r['events'] = {}
            for k, v in us.items():
                nb = (ev_arms[k][0] + 1.0) * B * C * Mp * 4
                r['events'][k] = dict(spread(v), bytes=nb, share_of_8TBs=nb / (np.median(v) * 1e-6) / HBM_SPEC,
                                      share_of_copy_rate=nb / (np.median(v) * 1e-6) / HBM_COPY)
            r['events']['indexed_over_plain'] = float(np.median(us['indexed fold=1']) / np.median(us['gather_windows']))

            def wall_ms(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)
            for k, fn in (('window_stats_ms', lambda: ops.window_stats(ws.planes, ws.rows, M, C)),
                          ('window_stats_indexed_ms', lambda: ops.window_stats_indexed(ws.planes, idx1, M, C, 1))):
                fn()
                r['events'][k] = spread([wall_ms(fn) for _ in range(max(5, args.rounds))])
        res[shape] = r
        del net, ws, x
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
