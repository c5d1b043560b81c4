"""What every analysis entry point does between its caller and its kernels, once: the list of runs normalised and checked,
one hashable group key per run, the device chosen, the runs staged as ``[Ttot, plane_stride(M)]`` float32 planes with the search
for non-finite values, and the planes handed out batch by batch of runs.  ``first_level``, ``single_trial``,
``searchlight_events``, ``crossnobis_events`` and ``connectivity_graph`` take all of it from here; an entry point brings its own
``who`` for the messages and nothing else.  ``aug_draw``, the NumPy restatement of the counter-based generator of
include/chebgcn.h, lives here as well, so that ``series`` and ``stats`` draw with one function.

Host-only at import: NumPy; torch and ``_lib`` are imported by the functions that need them.
"""
import numpy as np


def is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def cuda_device(device=None, like=None):
    """The device of a call: the one given, else that of the CUDA tensor ``like``, else the current one."""
    import torch
    if device is not None:
        return torch.device(device)
    if like is not None and is_tensor(like) and like.is_cuda:
        return like.device
    return torch.device('cuda', torch.cuda.current_device())


# ---- arguments ------------------------------------------------------------------------------------------------------------------

def as_runs(runs, who, min_rows=0, min_cols=1, **say):
    """One ``[T, M]`` run or a list of them -> ``(runs, single, M, all_tensors)``: a list of 2-d NumPy arrays and torch tensors of
    one width ``M >= min_cols`` and at least ``min_rows`` rows each, whether one run came bare, and whether every run is a tensor.
    ``say`` replaces the text of a refusal (``none``, ``shape``, ``width``, ``rows``) for a caller that words it otherwise."""
    say = dict(dict(none='no runs', shape='every run must be [T, M]', width='runs differ in the number of vertices (or have none)',
                    rows='every run needs at least %d rows' % min_rows), **say)
    single = isinstance(runs, np.ndarray) or is_tensor(runs)
    if single and runs.ndim != 2:
        raise ValueError('%s: a run must be [T, M], got shape %r' % (who, tuple(runs.shape)))
    runs = [runs] if single else list(runs)
    if not runs:
        raise ValueError('%s: %s' % (who, say['none']))
    tensors = all(is_tensor(r) for r in runs)
    runs = [r if is_tensor(r) else np.asarray(r) for r in runs]
    if any(r.ndim != 2 for r in runs):
        raise ValueError('%s: %s' % (who, say['shape']))
    M = int(runs[0].shape[1])
    if M < min_cols or any(int(r.shape[1]) != M for r in runs):
        raise ValueError('%s: %s' % (who, say['width']))
    if any(int(r.shape[0]) < min_rows for r in runs):
        raise ValueError('%s: %s' % (who, say['rows']))
    return runs, single, M, tensors


def group_keys(groups, R, who, what='run'):
    """One hashable key per run (``what``: or per sample) -> ``(groups as a list, the keys in order of first appearance, the
    members of every key in that order)``; ``None``: one group."""
    groups = [0] * R if groups is None else list(groups)
    if len(groups) != R:
        raise ValueError('%s: groups must hold one key per %s (%d %ss, %d keys)' % (who, what, R, what, len(groups)))
    keys, members = [], {}
    for r, g in enumerate(groups):
        try:
            hash(g)
        except TypeError:
            raise ValueError('%s: group key %r of %s %d is not hashable' % (who, g, what, r)) from None
        if g not in members:
            keys.append(g)
            members[g] = []
        members[g].append(r)
    return groups, keys, [members[g] for g in keys]


def host_array(y, who, any_dtype=False):
    """A series on the host as finite float32; ``any_dtype``: whatever NumPy casts to float32, not numbers only."""
    y = y.detach().cpu().numpy() if is_tensor(y) else np.asarray(y)
    if not any_dtype and y.dtype.kind not in 'fiu':
        raise ValueError('%s: series of dtype %s' % (who, y.dtype))
    y = y.astype(np.float32)
    if not np.isfinite(y).all():
        raise ValueError('%s: series hold non-finite values' % who)
    return y


# ---- planes ---------------------------------------------------------------------------------------------------------------------

def offsets(runs):
    """The first row of every run in the concatenation of the runs, and the total: int64 [R + 1]."""
    return np.concatenate([[0], np.cumsum([int(r.shape[0]) for r in runs])]).astype(np.int64)


def stage(runs, M, device, who, any_dtype=False):
    """The runs of ``as_runs`` as ``[Ttot, plane_stride(M)]`` float32 planes, run r at ``offsets(runs)[r]``, the padding columns
    zero: ``(device, planes)``.  The device is ``cuda_device(device, the first CUDA tensor among the runs)``.  Host arrays are
    checked (``host_array``) before the device is touched; tensors are staged where they lie, detached, and checked on the
    planes.  A non-finite value is a ``ValueError``."""
    host = [None if is_tensor(r) else host_array(r, who, any_dtype) for r in runs]
    import torch
    from . import _lib
    dev = cuda_device(device, next((r for r in runs if is_tensor(r) and r.is_cuda), None))
    offs = offsets(runs)
    shape = (int(offs[-1]), _lib.plane_stride(M))
    if all(h is not None for h in host):
        staged = np.zeros(shape, np.float32)
        for h, o in zip(host, offs):
            staged[o:o + h.shape[0], :M] = h
        return dev, torch.as_tensor(staged).to(dev)
    planes = torch.zeros(shape, dtype=torch.float32, device=dev)
    for y, h, o in zip(runs, host, offs):
        planes[o:o + y.shape[0], :M] = (y.detach() if h is None else torch.as_tensor(h)).to(dev, torch.float32)
    if not bool(torch.isfinite(planes).all()):
        raise ValueError('%s: series hold non-finite values' % who)
    return dev, planes


def batch_size(batch_runs, R, limit, run_bytes, device):
    """The runs of one pass of the kernels: ``batch_runs`` as given, by default what fits a quarter of the free device memory at
    ``run_bytes`` of workspace per run; at least 1, at most ``min(R, limit)``."""
    if batch_runs is None:
        import torch
        batch_runs = max(1, int(torch.cuda.mem_get_info(device)[0] // 4) // run_bytes)
    return int(min(batch_runs, R, limit))


def batches(planes, offs, batch_runs):
    """``(r0, r1, rows, o)`` batch by batch of ``batch_runs`` runs: the planes of runs ``r0 .. r1 - 1`` and their offsets inside
    ``rows``, int64 [r1 - r0 + 1] on the planes' device."""
    import torch
    R = len(offs) - 1
    for r0 in range(0, R, batch_runs):
        r1 = min(r0 + batch_runs, R)
        yield r0, r1, planes[int(offs[r0]):int(offs[r1])], torch.as_tensor(offs[r0:r1 + 1] - offs[r0]).to(planes.device)


# ---- the counter-based generator of include/chebgcn.h, restated in NumPy: uint32 values carried in uint64 and masked -------------
AUG_MUL1, AUG_MUL2, AUG_KEY, AUG_WINDOW = 0x7FEB352D, 0x846CA68B, 0x9E3779B9, 0x85EBCA6B
_U32 = np.uint64(0xFFFFFFFF)


def _aug_fin(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(AUG_MUL1)) & _U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(AUG_MUL2)) & _U32
    return x ^ (x >> np.uint64(16))


def aug_draw(seed, refill, i, d):
    """``chebgcn_aug_draw``: 32 uniform bits (in a uint64 array) for augmented windows ``i`` and draw indices ``d`` (arrays that
    broadcast), a stateless function of ``(seed, refill, i, d)``."""
    i = np.asarray(i, np.uint64) & _U32
    d = np.asarray(d, np.uint64) & _U32
    a = _aug_fin((_aug_fin(np.uint64(int(seed) & 0xFFFFFFFF)) + np.uint64(int(refill) & 0xFFFFFFFF)) & _U32)
    k0 = _aug_fin((a + i) & _U32)
    k1 = _aug_fin(((a ^ np.uint64(AUG_KEY)) + ((i * np.uint64(AUG_WINDOW)) & _U32)) & _U32)
    return _aug_fin(_aug_fin((k0 + d) & _U32) ^ k1)
