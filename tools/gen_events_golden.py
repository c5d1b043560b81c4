#!/usr/bin/env python3
"""Generate tests/golden/events_*.npz by RUNNING THE REFERENCE's ``matching_fmri_data_to_trials_event`` (utils.py:423-525).

The function is taken out of a reference checkout at run time (``ast``: its ``FunctionDef`` alone, compiled and executed with
NumPy, pandas and sklearn's ``preprocessing`` as its globals -- the module itself imports packages this tool does not need)
and called on small seeded designs.  Each file holds data only: the runs, their per-TR condition names, the settings of the
call, and what the function returned (windows ``[runs, S, M, channel]``, labels, ``Trial_dura``).  Under NumPy 2 the reference
runs only where every block of every run has the same length and every run yields the same number of windows (it builds
``np.array`` of the per-block lists), so every design here is regular in that sense; ragged designs are tested against a
restatement in tests/test_events_host.py.

    python tools/gen_events_golden.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import ast
import contextlib
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 5                                   # vertices
TARGETS = ['story', 'math', 'cue']      # (sorted: cue, math, story -- the label codes are not the order given)


def design(*parts):
    """('rest', 4), ('math', 8), ... -> the per-TR names."""
    return [name for name, n in parts for _ in range(n)]


def regular(order, gap=4, dura=8, tail=4):
    parts = [('rest', gap)]
    for i, name in enumerate(order):
        parts += [(name, dura), ('rest', tail if i == len(order) - 1 else gap)]
    return design(*parts)


R3 = [regular(['story', 'math', 'cue', 'math']), regular(['cue', 'story', 'math', 'story'], gap=3, tail=7)]
ADJ = [design(('rest', 3), ('story', 8), ('math', 8), ('rest', 4), ('cue', 8), ('story', 8), ('rest', 2), ('math', 8), ('rest', 5)),
       design(('rest', 5), ('cue', 8), ('story', 8), ('rest', 2), ('math', 8), ('cue', 8), ('rest', 4), ('story', 8), ('rest', 3))]
# two same-condition trials of 8 separated by rest merge into one block of 16: block_dura = 6 cuts a chunk across the gap
MERGE = [design(('rest', 4), ('story', 8), ('rest', 3), ('story', 8), ('rest', 4), ('math', 16), ('rest', 4), ('cue', 16), ('rest', 4)),
         design(('rest', 2), ('cue', 16), ('rest', 5), ('math', 8), ('rest', 2), ('math', 8), ('rest', 4), ('story', 16), ('rest', 6))]

CASES = {
    'base': dict(designs=R3, block_dura=4),
    'start_plus2': dict(designs=R3, block_dura=4, start_trial=2),
    'start_minus2': dict(designs=R3, block_dura=4, start_trial=-2),
    'remainder': dict(designs=R3, block_dura=6, flag_event=1),
    'clip': dict(designs=R3, block_dura=12, flag_event=1),
    'trstep2': dict(designs=R3, block_dura=4, TRstep=2),
    'adjacent': dict(designs=ADJ, block_dura=4),
    'hrf2': dict(designs=R3, block_dura=4, hrf_delay=2),
    'merge': dict(designs=MERGE, block_dura=6, flag_event=1),
    'merge_trstep3': dict(designs=MERGE, block_dura=6, flag_event=1, TRstep=3),
}


def reference_function(ref):
    import pandas as pd
    from sklearn import preprocessing
    path = os.path.join(ref, 'utils.py')
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'matching_fmri_data_to_trials_event']
    assert len(fn) == 1, 'matching_fmri_data_to_trials_event not found in %s' % path
    ns = {'np': np, 'pd': pd, 'preprocessing': preprocessing}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, 'exec'), ns)
    return ns['matching_fmri_data_to_trials_event']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference project (holds utils.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    match = reference_function(args.ref)
    codes = {n: i for i, n in enumerate(sorted(set(TARGETS)))}
    for k, (name, case) in enumerate(sorted(CASES.items())):
        case = dict(case)
        designs = case.pop('designs')
        rs = np.random.RandomState(100 + k)
        runs = [(rs.randn(len(d), M) * 3 + rs.randn(M)).astype(np.float32) for d in designs]
        kw = dict(block_dura=case['block_dura'], start_trial=case.get('start_trial', 0), hrf_delay=case.get('hrf_delay', 0),
                  flag_event=case.get('flag_event', 0), TRstep=case.get('TRstep', 1))
        with contextlib.redirect_stdout(io.StringIO()):
            x, y, names, trial_dura = match([r.copy() for r in runs], [list(d) for d in designs], list(TARGETS),
                                            ['run%d' % i for i in range(len(runs))], verbose=0, **kw)
        x, y = np.asarray(x), np.asarray(y)
        assert x.ndim == 4 and x.shape[:2] == y.shape and x.shape[2] == M and x.dtype == np.float32, (name, x.shape, x.dtype)
        fields = {'nruns': np.int64(len(runs)), 'target_name': np.array(TARGETS), 'windows': x,
                  'labels': np.vectorize(codes.get)(y).astype(np.int64), 'label_names': y.astype(str),
                  'trial_dura': np.int64(trial_dura), 'numpy_version': np.array(np.__version__)}
        for key, v in kw.items():
            fields[key] = np.int64(v)
        for i, (r, d) in enumerate(zip(runs, designs)):
            fields['run%d' % i] = r
            fields['design%d' % i] = np.array(d)
        path = os.path.join(args.out, 'events_%s.npz' % name)
        np.savez_compressed(path, **fields)
        print('%-14s %s windows %s  Trial_dura %d  -> %s (%d bytes)' % (name, kw, x.shape, trial_dura, path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
