"""Every arm of the bf16 matrix-core contraction at pool 1 and of its gradients (csrc/contract_bf16.hip) at the edges of its chunks
and tiles, against float64 NumPy restatements of the arithmetic each arm is meant to do.  Needs an MI355X: ``-m gpu``.

The C entries are called directly: chebgcn_contract_bwd_w_bf16, _bwd_w_bf16_dy16, chebgcn_contract_bwd_x_bf16, _bwd_x_bf16_dy16,
chebgcn_contract_fwd_bf16 (pool 1, with and without ReLU and its mask, the three bias kinds) and chebgcn_relu_grad_bf16 (the
round trip of the forward's own mask).  ``bwb_plan`` / ``bwd_x_waves`` / ``fwd_tiles`` / ``ksteps`` / ``lolo`` restate the dispatch
arithmetic for 256 CUs, the two gx knobs (CHEBGCN_BWB_GX, CHEBGCN_BWB_WIDE_GX) and the cap gx <= total included; every call asserts
that ``_lib.last_dispatch()`` is exactly the predicted string, the reduce kernels included, and ``test_tables_reach_every_arm``
asserts from the restatement alone that the case table reaches

    all 20 contract_bwd_w_bf16_kernel<RT,CT,P>; a ragged last row group (gy = 2: one live tile and four placeholder tiles), a
    ragged last column tile (gz = 2), Fin*K and Fout that are no multiples of 32, gx = 1, gx = total, and workgroups that stride
    over >= 3 chunks past a tail chunk and a window boundary, with the knob and without; the chunk whose upper half lies beyond
    the plane (Mp % 64 == 32);
    contract_bwd_w_bf16_wide_kernel<1>, <3> and <1,dy16>, each at 161 x 65, at gy = 2 (321 rows) and at gz = 2 (257 columns);
    chunk ranges of 1, 2, 3, 4 and >= 9 chunks per workgroup (the prologue's re-read, the ring wrap, a tail chunk followed by the
    next window's first chunk), M % 16 in {0, 1, 7, 8, 9, 15};
    bwb_reduce_stage1 with nx in {1, 7, 8, 9, 32, 33, 256, 257};
    contract_fwd_bf16_kernel<P,4> and <P,5> (P = 1, 3), <1,4,x16> and <1,5,x16> with the out_K scatter: Fin*K in {1, 63, 64, 65,
    256, 257, 300, 320, 321, 513}, Fout in {1, 15, 16, 17, 32, 33, 65}, K in {1, 2, 3, 4, 5, 6, 7, 25};
    the pool-1 forward's <P,4>, <P,4,tiles2>, <P,4,tiles4> (P = 1, 3) with the ReLU mask, every bias kind, both sides of lolo;
    more work items than the 256 persistent workgroups (forward and bwd_x), and the XCD-aware item order of a per-vertex bias.

Each case runs two legs through ``run_exact`` / ``run_roundoff``, which take the entries as an object: ``Device`` here, a NumPy
stand-in of the hi/lo arithmetic (with planted faults) in tests/test_contract_bf16_refs.py.

Exact leg: operand assignments whose every product and partial sum is exact, so that the result equals the restatement bit for
bit.  (a) both operands bf16-exact -- integers in [-4, 4], multiples of 1/8 in [-1, 1] -- for P = 1 and P = 3: this is what makes
the one-pass arms strict.  (b), P = 3: the first operand (the stack; dy for bwd_x) is +-(1 + j 2^-g), j odd, g = 8 ... 10: nine to
eleven significant bits, so hi = bf16(v) and lo = v - hi != 0 are both bf16-exact, lo of both signs; the other operand is
bf16-exact, so lo*lo = 0 and hi*hi + hi*lo + lo*hi is the full product.  (c): the reverse (W; dy for bwd_w) -- the lo image of
pack_w_bf16_kernel in both orientations.  (d), bwd_x and the forward at reductions of at most 33 rows: both operands carry low
parts (g = 8, magnitudes in [1, 1.5)): the full product where ``lolo`` holds (<= 32 rows), the full product minus sum lo*lo at 33.
``assert_exact_arithmetic`` proves per case and leg that the sum of the magnitudes of all terms is below 2^23 units of the finest
grain (one bit inside fp32): g is the largest of 10, 9, 8 for which that holds.  That the matrix cores accumulate such sums exactly
is an assumption (shown in this project for 14-bit sums only).  ``plant`` / ``census`` put and assert nonzero operands at vertex 0,
vertex M - 1, the first vertex of the last 16-chunk, 64-chunk and 128-tile, windows 0 and B - 1, the first and last row and column
of every tile and tile group and k-step, and at least half (here: all) of a low-carrying operand with lo != 0 of both signs.

Emulated round-off leg: standard-normal operands scaled as in test_split_bf16_arm_vs_float64, against the float64 sum of the
arithmetic the kernel is meant to do -- P = 1: the operands rounded to bf16 on the host (RNE); P = 3: hi*hi + hi*lo + lo*hi of the
host-side split, plus lo*lo where ``lolo`` holds -- so only fp32 accumulation error remains, and every arm, one-pass included, is
held to REL = 1e-5 (forward) and GREL = 2e-5 (gradients) of the reference's max (test_gpu_dispatch.py).  The comparison with the
plain float64 product stays as a second assertion at 1e-2 (P = 1) and 1e-5 (P = 3).
Measured on an MI355X over the table, worst error / bound against the emulation: forward 0.014 (1.4e-07, P = 3 on
f-B3-M129-13x5-F257-v; one pass 0.009, 9.3e-08 on f-B1-M127-5x7-F128-f), bwd_x 0.010 (2.0e-07, P = 3 on x-B3-M129-12x25-F65; one
pass 0.007, 1.4e-07 on the same case), bwd_w 0.016 (3.2e-07, P = 3 on w-B17-M65-5x7-F33-gx1; one pass 0.008, 1.5e-07 on
w-B3-M97-7x23-F65-gx9).  Against the plain product: one pass 0.33 ... 0.38 of 1e-2 (3.3e-03 bwd_w on w-B3-M97-7x23-F64, 3.5e-03
bwd_x on x-B2-M160-64x5-F1, 3.8e-03 forward on f-B1-M513-2x2-F8-f), three passes 0.60 ... 0.66 of 1e-5 (6.2e-06 bwd_w on
w-B17-M65-5x7-F33-gx33, 6.0e-06 bwd_x on x-B2-M129-107x3-F33, 6.6e-06 forward on f-B1-M127-5x7-F128-f).  Every exact leg held bit
for bit, sums of up to 2^23 units included.

Bit-identities, all exact: each launch runs twice into freshly poisoned buffers; the *_dy16 entries equal the fp32-dy entries at
passes = 1 on dy rounded to bf16; the dy16 chebgcn_relu_grad_bf16 writes from the forward's own mask is the RNE rounding of
mask ? dout : 0; the mask is out > 0 over [0, M); chebgcn_contract_bwd_w_bf16_dy16 refuses ('only for wide layers') exactly where
chebgcn_bf16_dy16_supported is 0.  Pads and bounds: every input pad [M, Mp) -- stack, dy, dy16, the per-vertex bias -- is NaN in
one run and +-1e30 in another; every output (dW, gstack [K][B][Fin][Mp], out, the mask, dy16) sits between sentinels; the workspace
is exactly the *_workspace() byte count followed by a sentinel; dW and the data columns of the float outputs are finite; nothing
is asserted about the values of output pads.
"""
import collections
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import record_measured
from gcn_fmri_decoding_amd import _lib
from gcn_fmri_decoding_amd._lib import BIAS_FILTER, BIAS_NONE, BIAS_VERTEX, plane_stride

import test_gpu_contract_grad_arms as T
from test_gpu_contract_grad_arms import (ASSUMES, CUS, GREL, GUARD, REL, _bits_equal, _flat, _twice, dW_ref, gstack_ref, inside,
                                         new_out, out_ref, pre_ref, rows_of, sums_ref, unpack_mask)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
N, F, V = BIAS_NONE, BIAS_FILTER, BIAS_VERTEX
BF16_REL = 1e-2           # one pass against the plain product (test_gpu_dispatch.py BF16_REL)
SPLIT_REL = 1e-5          # three passes against the plain product (test_split_bf16_arm_vs_float64)
KNOB_TILED, KNOB_WIDE = 'CHEBGCN_BWB_GX', 'CHEBGCN_BWB_WIDE_GX'
U16 = np.dtype(np.uint16)
T.SENT.setdefault(U16, 0xA5A5)                               # dy16 buffers between sentinels (new_out / inside)
T.POISON.setdefault(U16, 0x5A5A)


# ------------------------------------------------------------------------------------------------------------ bf16 on the host

def bf16_round(a):
    """fp32 -> the nearest bf16 (RNE, torch's conversion), as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_bits(a):
    """fp32 -> the bits of the nearest bf16 (uint16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bits_f32(u):
    """bf16 bits -> fp32"""
    return (np.ascontiguousarray(u).astype(np.uint32) << 16).view(np.float32)


def split(a):
    """x -> (hi, lo) float64: hi = bf16(x), lo = bf16(x - hi), as pack_w_bf16_kernel and the operand conversions do"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = bf16_round(a)
    return hi.astype(np.float64), bf16_round(a - hi).astype(np.float64)


def emu(A, Bm, passes, lolo=False, zero_lo=(False, False), lolo_extra=False):
    """float64 A @ Bm of what a P-pass kernel multiplies.  zero_lo / lolo_extra: planted faults of the stand-in."""
    (ah, al), (bh, bl) = split(A), split(Bm)
    if passes == 1:
        return ah @ bh
    al, bl = (0 * al if zero_lo[0] else al), (0 * bl if zero_lo[1] else bl)
    r = ah @ bh + ah @ bl + al @ bh
    return r + al @ bl if (lolo or lolo_extra) else r


# ------------------------------------------------------------------------------------------------------------ dispatch restatement

def ksteps(n):
    return (n + 15) // 16


def lolo(passes, reduction):
    """CG_BF16_LOLO_KSTEPS = 2: reductions of at most 32 rows keep lo*lo (contract_fwd_bf16_kernel: the forward and bwd_x)"""
    return passes == 3 and ksteps(reduction) <= 2


def fwd_tiles(Fout):
    return 4 if Fout <= 64 else 2 if Fout <= 128 else 1


def bwd_x_waves(rows):
    return 5 if (rows + 319) // 320 * 320 < (rows + 255) // 256 * 256 else 4


Plan = collections.namedtuple('Plan', 'wide rt ct gx gy gz per total chunk')


def bwb_plan(B, M, FinK, Fout, gx_tiled=None, gx_wide=None):
    """bwb_plan of contract_bf16.hip; gx_tiled / gx_wide: the values of CHEBGCN_BWB_GX / CHEBGCN_BWB_WIDE_GX (None: unset)"""
    if FinK > 160 and Fout > 64:
        gy, gz = (FinK + 319) // 320, (Fout + 255) // 256
        total = B * ((M + 15) // 16)
        gx = CUS // (gy * gz)
        if gx_wide and gx_wide > 0:
            gx = gx_wide
        return Plan(True, 10, 8, max(1, min(gx, total)), gy, gz, 10 * 8 * 16 * 64, total, 16)
    ntiles = (FinK + 31) // 32
    rt, ct = min(ntiles, 5), 2 if Fout > 32 else 1
    gy, gz = (ntiles + rt - 1) // rt, (Fout + 32 * ct - 1) // (32 * ct)
    total = B * ((M + 63) // 64)
    gx = (2 * CUS // (gy * gz) + 127) // 128 * 128
    gx = max(CUS // 2, min(gx, 2 * CUS))
    if gy * gz >= 8:
        gx = max(1, 2 * CUS // (gy * gz))
    if gx_tiled and gx_tiled > 0:
        gx = gx_tiled
    return Plan(False, rt, ct, max(1, min(gx, total)), gy, gz, rt * ct * 16 * 64, total, 64)


def bwb_workspace(p):
    return (p.gx + 8) * p.gy * p.gz * p.per * 4


def bwd_x_workspace(FinK, Fout):
    G = 64 * bwd_x_waves(FinK)
    return 2 * ksteps(Fout) * ((FinK + G - 1) // G * G) * 16 * 2


def fwd_workspace(FinK, Fout):
    return 2 * ksteps(FinK) * ((Fout + 255) // 256 * 256) * 16 * 2


def chunk_ranges(p):
    """chunks each workgroup of bwd_w walks: wide -- the sizes of its contiguous ranges; tiled -- the chunks of its stride"""
    if p.wide:
        return [p.total * (x + 1) // p.gx - p.total * x // p.gx for x in range(p.gx)]
    return [len(range(x, p.total, p.gx)) for x in range(p.gx)]


_REDUCE = ' + bwb_reduce_stage1 + bwb_reduce_stage2'


def bwd_w_arm(p, passes, dy16=False):
    if p.wide:
        return 'contract_bwd_w_bf16_wide_kernel<%s>' % ('1,dy16' if dy16 else passes) + _REDUCE
    return 'contract_bwd_w_bf16_kernel<%d,%d,%d>' % (p.rt, p.ct, passes) + _REDUCE


def bwd_x_arm(FinK, passes, x16=False):
    return 'pack_w_bf16_kernel<transposed> + contract_fwd_bf16_kernel<%d,%d%s>' % (passes, bwd_x_waves(FinK), ',x16' if x16 else '')


def fwd_arm(Fout, passes):
    return 'pack_w_bf16_kernel + contract_fwd_bf16_kernel<%d,4%s>' % (passes, {4: ',tiles4', 2: ',tiles2', 1: ''}[fwd_tiles(Fout)])


def relu_grad16_arm(M, Fout):
    return 'bias_grad_relu_kernel<CHEBGCN_BIAS_NONE,%d,bf16>' % T.bias_grad_blocks(M, Fout)[1]


# ------------------------------------------------------------------------------------------------------------ the case table

# kind: 'w' chebgcn_contract_bwd_w_bf16(_dy16), 'x' chebgcn_contract_bwd_x_bf16(_dy16), 'f' chebgcn_contract_fwd_bf16 at pool 1
# bias: the forward's bias kind; gx: the value of the gx knob of the case's bwd_w kernel (None: unset, the production plan)
Case = collections.namedtuple('Case', 'kind B M Fin K Fout bias gx')


def _w(B, M, Fin, K, Fout, gx=None):
    return Case('w', B, M, Fin, K, Fout, N, gx)


def _x(B, M, Fin, K, Fout):
    return Case('x', B, M, Fin, K, Fout, N, None)


def _f(B, M, Fin, K, Fout, bias):
    return Case('f', B, M, Fin, K, Fout, bias, None)


TABLE = [
    # ---- tiled bwd_w, the production plan: (rt, ct) and what is ragged.  B * ceil(M / 64) <= 6 workgroups: gx = total
    _w(1, 1, 1, 1, 1),                 # <1,1>: one term
    _w(2, 31, 5, 7, 33),               # <2,2>: 35 rows, the second column tile holds one column
    _w(3, 32, 3, 23, 32),              # <3,1>: 69 rows
    _w(2, 33, 4, 25, 65),              # <4,2>: gz = 2, the second column group holds one column
    _w(3, 63, 5, 32, 17),              # <5,1>: 160 rows, the most one row group holds
    _w(1, 64, 11, 3, 31),              # <2,1>: a full chunk, no tail
    _w(2, 65, 1, 17, 64),              # <1,2>: Mp = 96, the upper half of the second chunk lies beyond the plane
    _w(3, 95, 7, 13, 40),              # <3,2>: Mp = 96
    _w(2, 96, 32, 4, 5),               # <4,1>: Mp = 96, M = Mp
    _w(3, 97, 7, 23, 64),              # <5,2>: 161 rows, gy = 2: the second group holds one live row tile and four placeholders
    _w(1, 97, 6, 32, 33),              # <5,2>: 192 rows, gy = 2
    _w(22, 129, 11, 3, 1000),          # <2,2>: gz = 16 -> 32 workgroups for 66 chunks: strides of 3 chunks without the knob; Mp = 160
    # ---- tiled bwd_w, gx by the knob: the reducer's nx, gx = 1, strides past tail chunks and windows (Mp = 96)
    _w(17, 65, 5, 7, 33, 1), _w(17, 65, 5, 7, 33, 7), _w(17, 65, 5, 7, 33, 8), _w(17, 65, 5, 7, 33, 9),
    _w(17, 65, 5, 7, 33, 32), _w(17, 65, 5, 7, 33, 33),
    _w(2, 33, 4, 25, 65, 500),         # the cap: gx = total = 2
    # ---- wide bwd_w, the production plan
    _w(3, 97, 7, 23, 65),              # 161 x 65, the smallest; M % 16 = 1; one chunk per workgroup
    _w(2, 40, 3, 107, 65),             # 321 rows: gy = 2, the second group holds one live row; M % 16 = 8
    _w(2, 55, 7, 23, 257),             # 257 columns: gz = 2; M % 16 = 7
    _w(40, 97, 3, 107, 257),           # gy = gz = 2 -> 64 workgroups for 280 chunks: ranges of 4 and 5 without the knob
    _w(13, 305, 7, 23, 65),            # 260 chunks: nx = 256
    _w(13, 305, 7, 23, 65, 257),       # nx = 257
    # ---- wide bwd_w, gx by the knob: ranges of 1, 2, 3, 4 and >= 9 chunks
    _w(3, 97, 7, 23, 65, 2),           # 21 chunks: ranges of 10 and 11: a tail chunk of one vertex, then the next window's first
    _w(3, 96, 7, 23, 65, 5),           # 18 chunks, M % 16 = 0: ranges of 3 and 4
    _w(3, 105, 23, 7, 65, 7),          # 21 chunks, M % 16 = 9: ranges of 3
    _w(3, 111, 7, 23, 65, 8),          # M % 16 = 15: ranges of 2 and 3
    _w(3, 97, 7, 23, 65, 9),
    _w(2, 55, 7, 23, 257, 300),        # the cap: gx = total = 8
    # ---- bwd_x: rows Fin*K, the reduction Fout, K of the scatter
    _x(1, 1, 1, 1, 1),
    _x(2, 3, 9, 7, 15),
    _x(3, 4, 32, 2, 16),
    _x(2, 5, 13, 5, 17),
    _x(1, 127, 64, 4, 32),             # lolo at its limit
    _x(2, 128, 257, 1, 33),            # five waves; the twin of lolo: 33 rows
    _x(3, 129, 12, 25, 65),
    _x(2, 160, 64, 5, 1),              # 320 rows: one full group of five waves
    _x(2, 129, 107, 3, 33),            # 321 rows: two groups of 256, the second holds 65
    _x(1, 160, 171, 3, 16),            # 513 rows: two groups of 320
    _x(2, 127, 50, 6, 17),
    _x(300, 5, 13, 5, 17),             # 300 work items for 256 persistent workgroups: 44 of them take a second item
    # ---- the forward at pool 1: tiles4 (Fout <= 64), tiles2 (<= 128), one tile
    _f(1, 1, 1, 1, 1, V),
    _f(2, 3, 3, 5, 33, N),
    _f(3, 4, 4, 8, 64, F),             # 32 rows: lolo at its limit
    _f(2, 5, 11, 3, 65, V),            # 33 rows: the twin
    _f(1, 127, 5, 7, 128, F),
    _f(2, 128, 2, 25, 129, N),
    _f(3, 129, 13, 5, 257, V),         # two filter groups, the second holds one filter
    _f(1, 160, 7, 3, 40, V),
    _f(2, 160, 17, 1, 100, N),
    _f(1, 513, 2, 2, 8, F),            # tiles4: two work items along the vertices, the second holds one vertex
    _f(2, 129, 3, 11, 200, F),
    _f(300, 5, 3, 5, 33, F),           # 300 work items for 256 workgroups: the ring runs on into a second item
    _f(33, 900, 2, 2, 129, V),         # eight vertex tiles and 264 items: the XCD-aware item order of a per-vertex bias
]
CASES = TABLE


def case_id(c):
    return '%s-B%d-M%d-%dx%d-F%d%s%s' % (c.kind, c.B, c.M, c.Fin, c.K, c.Fout, '-' + 'nfv'[c.bias] if c.kind == 'f' else '',
                                         '-gx%d' % c.gx if c.gx else '')


def plan_of(c):
    wide = c.Fin * c.K > 160 and c.Fout > 64
    return bwb_plan(c.B, c.M, c.Fin * c.K, c.Fout, None if wide else c.gx, c.gx if wide else None)


def knobs_of(c):
    """{knob: value or None} for the case: its own knob, and the other kernel's set to a value that must be ignored"""
    wide = c.kind == 'w' and plan_of(c).wide
    mine, other = (KNOB_WIDE, KNOB_TILED) if wide else (KNOB_TILED, KNOB_WIDE)
    return {mine: str(c.gx) if c.gx else None, other: str(c.gx + 3) if c.gx else None}


def set_knobs(monkeypatch, c):
    for k, v in knobs_of(c).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def reduction(c):
    return {'w': c.B * c.M, 'x': c.Fout, 'f': c.Fin * c.K}[c.kind]


def legs_of(c):
    """[(leg, passes ...)] of the exact leg"""
    legs = [('a', (1, 3)), ('b', (3,)), ('c', (3,))]
    if c.kind in 'xf' and reduction(c) <= 33:
        legs.append(('d', (3,)))
    return legs


def table_reach(table=None):
    """What the table (default: TABLE) reaches by the dispatch restatement (no device): asserts the list in the module docstring."""
    tiled, wide, nx, rows_x, fout_x, ks_x, bwx, fwd = set(), set(), set(), set(), set(), set(), set(), set()
    r = collections.Counter()
    wide_ranges = {}
    for c in (TABLE if table is None else table):
        FinK = c.Fin * c.K
        if c.kind == 'w':
            p = plan_of(c)
            ranges = chunk_ranges(p)
            assert sum(ranges) == p.total and p.gx <= p.total, c
            nx.add(p.gx)
            nat = c.gx is None
            if p.wide:
                shape = (FinK == 161 and c.Fout == 65, p.gy == 2, p.gz == 2)
                for passes, dy16 in ((1, False), (3, False), (1, True)):
                    arm = bwd_w_arm(p, passes, dy16).split(' + ')[0]
                    wide.update((arm, s) for s, on in zip(('smallest', 'gy2', 'gz2'), shape) if on)
                wide_ranges.setdefault(nat, set()).update(ranges)
                r['wide M%%16=%d' % (c.M % 16)] += 1
                # a range that holds a tail chunk followed by the next window's first chunk
                r['wide tail then window'] += c.M % 16 != 0 and max(ranges) > (c.M + 15) // 16
                r['wide natural multi-chunk'] += nat and max(ranges) >= 2
            else:
                tiled.update((p.rt, p.ct, passes) for passes in (1, 3))
                ntiles = (FinK + 31) // 32
                r['tiled ragged gy'] += p.gy > 1 and ntiles % p.rt == 1 and p.rt == 5 and c.Fout <= 64
                r['tiled ragged gz'] += p.gz > 1 and c.Fout == 65 and FinK <= 160
                r['tiled odd sizes'] += FinK % 32 != 0 and c.Fout % 32 != 0
                r['tiled gx=1'] += p.gx == 1 and p.total > 1
                r['tiled gx=total'] += p.gx == p.total > 1
                # a workgroup of >= 3 chunks, a tail chunk among them, in more than one window
                ncm = (c.M + 63) // 64
                walks = [range(x, p.total, p.gx) for x in range(p.gx)]
                stride = c.M % 64 != 0 and any(len(w) >= 3 and any(i % ncm == ncm - 1 for i in w) and len({i // ncm for i in w}) >= 2
                                               for w in walks)
                r['tiled stride'] += stride
                r['tiled natural stride'] += stride and nat and c.B * ((c.M + 63) // 64) > p.gx
                r['tiled beyond the plane'] += plane_stride(c.M) % 64 == 32
                r['tiled M=%d' % c.M] += 1
        elif c.kind == 'x':
            rows_x.add(FinK), fout_x.add(c.Fout), ks_x.add(c.K)
            bwx.update(bwd_x_arm(FinK, passes, x16).split(' + ')[1] for passes, x16 in ((1, False), (3, False), (1, True)))
            r['x M=%d' % c.M] += 1
            r['x lolo'] += lolo(3, c.Fout)
            r['x not lolo'] += not lolo(3, c.Fout)
            G = 64 * bwd_x_waves(FinK)
            r['x second item'] += (c.M + 127) // 128 * c.B * ((FinK + G - 1) // G) > CUS
        else:
            fwd.update((fwd_arm(c.Fout, passes).split(' + ')[1], c.bias) for passes in (1, 3))
            r['f M=%d' % c.M] += 1
            r['f lolo'] += lolo(3, FinK)
            r['f twin'] += FinK == 33
            nvt = fwd_tiles(c.Fout)
            ntm = (c.M + 128 * nvt - 1) // (128 * nvt)
            items = ntm * c.B * ((c.Fout + 256 // nvt - 1) // (256 // nvt))
            r['f second item'] += items > CUS
            r['f XCD order'] += items > CUS and c.bias == V and ntm >= 8
    assert tiled == {(rt, ct, passes) for rt in range(1, 6) for ct in (1, 2) for passes in (1, 3)}, sorted(tiled)
    for key in ('tiled ragged gy', 'tiled ragged gz', 'tiled odd sizes', 'tiled gx=1', 'tiled gx=total', 'tiled stride',
                'tiled natural stride', 'tiled beyond the plane', 'wide tail then window', 'wide natural multi-chunk', 'x lolo',
                'x not lolo', 'f lolo', 'f twin', 'x second item', 'f second item', 'f XCD order'):
        assert r[key] >= 1, key
    assert all(r['tiled M=%d' % m] for m in (1, 31, 32, 33, 63, 64, 65, 95, 96, 97)), r
    assert all(r['wide M%%16=%d' % m] for m in (0, 1, 7, 8, 9, 15)), r
    assert all(r['x M=%d' % m] for m in (1, 3, 4, 5, 127, 128, 129, 160)), r
    assert all(r['f M=%d' % m] for m in (1, 3, 4, 5, 127, 128, 129, 160)), r
    arms = ('contract_bwd_w_bf16_wide_kernel<1>', 'contract_bwd_w_bf16_wide_kernel<3>', 'contract_bwd_w_bf16_wide_kernel<1,dy16>')
    assert wide == {(a, s) for a in arms for s in ('smallest', 'gy2', 'gz2')}, sorted(wide)
    both = wide_ranges[True] | wide_ranges[False]
    assert {1, 2, 3, 4} <= both and max(both) >= 9, sorted(both)
    assert {1, 7, 8, 9, 32, 33, 256, 257} <= nx, sorted(nx)
    assert bwx == {'contract_fwd_bf16_kernel<%s>' % a for a in ('1,4', '3,4', '1,5', '3,5', '1,4,x16', '1,5,x16')}, sorted(bwx)
    assert rows_x >= {1, 63, 64, 65, 256, 257, 300, 320, 321, 513}, sorted(rows_x)
    assert fout_x >= {1, 15, 16, 17, 32, 33, 65} and ks_x >= {1, 2, 3, 4, 5, 6, 7, 25}, (sorted(fout_x), sorted(ks_x))
    geoms = {'contract_fwd_bf16_kernel<%d,4%s>' % (passes, t) for passes in (1, 3) for t in ('', ',tiles2', ',tiles4')}
    assert {a for a, _ in fwd} == geoms and {b for _, b in fwd} == {N, F, V}, sorted(fwd)
    assert all({b for a, b in fwd if a == g} == {N, F, V} for g in geoms), sorted(fwd)
    return dict(tiled=sorted('<%d,%d,%d>' % a for a in tiled), wide=sorted('%s %s' % a for a in wide), nx=sorted(nx),
                wide_ranges=sorted(both), bwd_x=sorted(bwx), fwd=sorted(geoms))


# ------------------------------------------------------------------------------------------------------------ exactness

LOW_TOP = {'b': 2.0, 'c': 2.0, 'd': 1.5}                     # magnitudes of a low-carrying operand: [1, top)


def _budget(c, leg, g):
    """An upper bound of the sum of the magnitudes of all terms of one output (every partial sum, in any order and of any subset
    of the passes, lies below it) in units of the finest grain of the leg.  Operands: integers |v| <= 4 (grain 1); eighths
    |v| <= 1 (grain 1/8); low-carrying |hi| + |lo| <= top + 2^-8 (grain 2^-g; hi*hi, hi*lo and lo*lo terms are multiples of
    2^-14, 2^-(7+g), 2^-2g: of 2^-2g, the grain of a leg where both operands carry low parts)."""
    first, second = ((4.0, 1.0), (4.0, 1.0)) if c.kind == 'w' else ((4.0, 1.0), (1.0, 0.125))     # (magnitude, grain)
    low = (LOW_TOP.get(leg, 0) + 2.0 ** -8, 2.0 ** -g)
    if leg in 'bd':
        first = low
    if leg in 'cd':
        second = low
    bias = 1.0 if c.kind == 'f' and c.bias != N else 0.0       # an eighth in [-1, 1]
    return (first[0] * second[0] * reduction(c) + bias) / (first[1] * second[1])


def grid_bits(c, leg):
    """g of the leg's low-carrying operand(s): the finest of 2^-10, 2^-9, 2^-8 that keeps every sum exact; 0 where there is none"""
    if leg == 'a':
        return 0
    for g in ((8,) if leg == 'd' else (10, 9, 8)):
        if _budget(c, leg, g) < 2 ** 23:
            return g
    raise AssertionError('%s leg %s: no grid of nine significant bits keeps the sums exact' % (case_id(c), leg))


def assert_exact_arithmetic(c):
    """Every partial sum of every leg stays below 2^23 units of the leg's grain: one bit inside fp32."""
    for leg, _ in legs_of(c):
        g = grid_bits(c, leg)
        assert leg == 'a' or 8 <= g <= 10, (c, leg)
        assert _budget(c, leg, g) < 2 ** 23, (c, leg, g)


# ------------------------------------------------------------------------------------------------------------ inputs

Inputs = collections.namedtuple('Inputs', 'stack W bias dy dout')         # padded fp32; what the kind does not read is None
PADS = {'a': ('nan', 'big'), 'b': ('nan',), 'c': ('big',), 'd': ('nan',), 'r': ('nan',)}


def special_vertices(M):
    """vertex 0, vertex M - 1 and the first vertex of the last 16-chunk, 64-chunk and 128-tile"""
    last = M - 1
    return sorted({0, last, last // 16 * 16, last // 64 * 64, last // 128 * 128})


def edges(n, *units):
    """the first and the last index of every block of ``u`` consecutive indices in [0, n), for every unit u"""
    e = {0, n - 1}
    for u in units:
        e.update(range(0, n, u))
        e.update(min(i + u, n) - 1 for i in range(0, n, u))
    return sorted(e)


def plant_sets(c):
    """(windows, vertices, rows of the Fin*K axis, indices of the Fout axis) where operands must be nonzero"""
    FinK = c.Fin * c.K
    if c.kind == 'w':
        p = plan_of(c)
        rows, cols = edges(FinK, 32, 320 if p.wide else 32 * p.rt), edges(c.Fout, 32, 256 if p.wide else 32 * p.ct)
    elif c.kind == 'x':
        rows, cols = edges(FinK, 64, 64 * bwd_x_waves(FinK)), edges(c.Fout, 16)
    else:
        rows, cols = edges(FinK, 16), edges(c.Fout, 64, 256 // fwd_tiles(c.Fout))
    return sorted({0, c.B - 1}), special_vertices(c.M), rows, cols


def _nonzero(a, *ix):
    sub = a[np.ix_(*ix)]
    a[np.ix_(*ix)] = np.where(sub == 0, 1, sub)


def plant(c, inp):
    bs, vs, rows, cols = plant_sets(c)
    if inp.stack is not None:
        ks, fins = [r % c.K for r in rows], [r // c.K for r in rows]
        for k, fin in zip(ks, fins):
            _nonzero(inp.stack, [k], bs, [fin], vs)
    if inp.W is not None:
        _nonzero(inp.W, rows, cols)
    if inp.dy is not None:
        _nonzero(inp.dy, bs, cols, vs)


def _seed(c, leg, pad):
    return zlib.crc32(('%s %s %s' % (case_id(c), leg, pad)).encode()) % (2 ** 31)


def _fill_pad(a, M, pad):
    n = a.shape[-1] - M
    a[..., M:] = np.nan if pad == 'nan' else (1e30 * (-1.0) ** np.arange(n)).astype(np.float32)


def make_inputs(c, leg, pad='nan'):
    """Padded fp32 arrays of leg 'a' ... 'd' (exact) or 'r' (round-off): stack [K, B, Fin, Mp], W [Fin*K, Fout], bias, dy
    [B, Fout, Mp], and for the forward dout [B, Fout, Mp] (standard normal: what chebgcn_relu_grad_bf16 rounds).  Every pad
    [M, Mp) holds NaN or +-1e30."""
    B, M, Fin, K, Fout = c[1:6]
    Mp, FinK = plane_stride(M), Fin * K
    rs = np.random.RandomState(_seed(c, leg, pad))
    g = 0 if leg == 'r' else grid_bits(c, leg)

    def ints(shape):
        return rs.randint(-4, 5, shape).astype(np.float32)

    def eighths(shape):
        return rs.randint(-8, 9, shape).astype(np.float32) * np.float32(0.125)

    def low(shape):
        j = 2 * rs.randint(0, int((LOW_TOP[leg] - 1) * 2 ** (g - 1)), shape) + 1
        return ((1 + j * 2.0 ** -g) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)

    def normal(shape, scale=1.0):
        return (rs.standard_normal(shape) * scale).astype(np.float32)

    first = normal if leg == 'r' else low if leg in 'bd' else ints
    stack = first((K, B, Fin, Mp)) if c.kind in 'wf' else None
    if c.kind == 'w':
        dy = (normal if leg == 'r' else low if leg in 'cd' else ints)((B, Fout, Mp))
    elif c.kind == 'x':
        dy = first((B, Fout, Mp))
    else:
        dy = None
    W = None
    if c.kind in 'xf':
        W = normal((FinK, Fout), 0.5 / np.sqrt(FinK)) if leg == 'r' else (low if leg in 'cd' else eighths)((FinK, Fout))
    bias = dout = None
    if c.kind == 'f':
        bshape = {N: None, F: (Fout,), V: (Fout, Mp)}[c.bias]
        if bshape:
            bias = normal(bshape, 0.3) if leg == 'r' else eighths(bshape)
        dout = normal((B, Fout, Mp))
    inp = Inputs(stack, W, bias, dy, dout)
    if leg != 'r':
        plant(c, inp)
    for a in (stack, dy, dout) + ((bias,) if c.bias == V else ()):
        if a is not None:
            _fill_pad(a, M, pad)
    return inp


def low_census(what, a):
    """a low-carrying operand: hi and lo bf16-exact, lo != 0 on at least half of the data with both signs"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = bf16_round(a)
    lo = a - hi
    assert np.array_equal(bf16_round(lo), lo), what + ': a low part that is not bf16-exact'
    assert 2 * np.count_nonzero(lo) >= lo.size, what + ': fewer than half of the low parts are nonzero'
    assert lo.size < 16 or ((lo > 0).any() and (lo < 0).any()), what + ': low parts of one sign only'
    return lo


def census(c, leg, inp, pad='nan'):
    """The plants hold: nonzero operands at the special vertices of windows 0 and B - 1 on the edges of every tile, group and
    k-step; the low-carrying operands carry low parts (there as well); every pad holds the pad value."""
    what = '%s leg %s' % (case_id(c), leg)
    M = c.M
    bs, vs, rows, cols = plant_sets(c)
    seen = {}
    if inp.stack is not None:
        S = rows_of(inp.stack[..., :M]).reshape(c.Fin * c.K, c.B, M)
        assert S[np.ix_(rows, bs, vs)].all(), what + ': a zero operand at a planted place of the stack'
    if inp.W is not None:
        assert inp.W[np.ix_(rows, cols)].all(), what + ': a zero operand at a planted place of W'
    if inp.dy is not None:
        assert inp.dy[np.ix_(bs, cols, vs)].all(), what + ': a zero operand at a planted place of dy'
    first = inp.dy if c.kind == 'x' else inp.stack
    second = inp.dy if c.kind == 'w' else inp.W
    for name, a, legs in (('first', first, 'bd'), ('second', second, 'cd')):
        data = a[..., :M] if a is not inp.W else a
        if leg in legs:
            lo = low_census('%s, the %s operand' % (what, name), data)
            corner = lo[np.ix_(rows, cols)] if a is inp.W else (lo[np.ix_(bs, cols, vs)] if a is inp.dy else
                                                              rows_of(lo).reshape(c.Fin * c.K, c.B, M)[np.ix_(rows, bs, vs)])
            assert corner.all(), what + ': a planted corner without a low part'
            seen[name + '_lo'] = int(np.count_nonzero(lo))
        else:
            assert np.array_equal(bf16_round(data), data), '%s: the %s operand is not bf16-exact' % (what, name)
    for a in (inp.stack, inp.dy, inp.dout) + ((inp.bias,) if c.bias == V else ()):
        if a is not None and a.shape[-1] > M:
            tail = a[..., M:]
            assert np.isnan(tail).all() if pad == 'nan' else (np.abs(tail) == np.float32(1e30)).all(), what + ': a pad'
    return seen


# ------------------------------------------------------------------------------------------------------------ restatements

def dW_emu(c, inp, passes, **fault):
    return emu(rows_of(inp.stack[..., :c.M]), _flat(inp.dy[..., :c.M]).T, passes, **fault)


def gstack_emu(c, inp, passes, **fault):
    """[K, B, Fin, M]: the out_K scatter of row r = fin*K + k to plane (k, b, fin)"""
    r = emu(inp.W, _flat(inp.dy[..., :c.M]), passes, lolo(passes, c.Fout), **fault)
    return r.reshape(c.Fin, c.K, c.B, c.M).transpose(1, 2, 0, 3)


def pre_emu(c, inp, passes, **fault):
    """[B, Fout, M]: the sums plus the bias, before the ReLU"""
    r = emu(np.ascontiguousarray(inp.W.T), rows_of(inp.stack[..., :c.M]), passes, lolo(passes, c.Fin * c.K), **fault)
    return pre_ref(r.reshape(c.Fout, c.B, c.M).transpose(1, 0, 2), c.bias, inp.bias)


def plain(c, inp):
    """the float64 product of the fp32 operands"""
    M = c.M
    if c.kind == 'w':
        return dW_ref(rows_of(inp.stack[..., :M]), inp.dy[..., :M])
    if c.kind == 'x':
        return gstack_ref(inp.W, inp.dy[..., :M], c.Fin, c.K)
    return pre_ref(sums_ref(rows_of(inp.stack[..., :M]), inp.W, c.B, M), c.bias, inp.bias)


def lolo_term(c, inp):
    """sum lo*lo of the operands, in the layout of ``plain``"""
    M = c.M
    if c.kind == 'x':
        r = split(inp.W)[1] @ split(_flat(inp.dy[..., :M]))[1]
        return r.reshape(c.Fin, c.K, c.B, M).transpose(1, 2, 0, 3)
    r = split(np.ascontiguousarray(inp.W.T))[1] @ split(rows_of(inp.stack[..., :M]))[1]
    return r.reshape(c.Fout, c.B, M).transpose(1, 0, 2)


EMU = {'w': dW_emu, 'x': gstack_emu, 'f': pre_emu}


def exact_ref(c, leg, inp, passes):
    """The restatement of an exact leg, after asserting that it is what the leg's design says: the full product, or (leg d beyond
    lolo) the full product minus sum lo*lo, which must differ from it."""
    ref, full = EMU[c.kind](c, inp, passes), plain(c, inp)
    if leg == 'd' and not lolo(passes, reduction(c)):
        assert np.array_equal(ref, full - lolo_term(c, inp)) and (ref != full).any(), case_id(c) + ': the twin of lolo'
    else:
        assert np.array_equal(ref, full), '%s leg %s: the arithmetic of %d passes is not the full product' % (case_id(c), leg, passes)
    return ref


# ------------------------------------------------------------------------------------------------------------ the two legs

def _launch(E, c, inp, passes, relu=1):
    """one launch of the case's entry: a tuple of outputs"""
    if c.kind == 'w':
        return (E.bwd_w(c, inp.stack, inp.dy, passes),)
    if c.kind == 'x':
        return (E.bwd_x(c, inp.dy, inp.W, passes),)
    return E.fwd(c, inp.stack, inp.W, inp.bias, relu, passes)


def _launch16(E, c, inp, d16):
    """the dy16 entry of a gradient on the bf16 bits d16: (rc, output, message)"""
    if c.kind == 'w':
        return E.bwd_w_dy16(c, inp.stack, d16)
    return 0, E.bwd_x_dy16(c, d16, inp.W), ''


def _dy16_identity(E, c, what, inp, one_pass):
    """the dy16 entry on dy rounded to bf16 (its pad rounded too) equals the fp32-dy entry at passes = 1, bit for bit; bwd_w refuses
    exactly where chebgcn_bf16_dy16_supported says so"""
    d16 = bf16_bits(inp.dy)
    ncol = c.M if c.kind == 'x' else None
    if c.kind == 'w' and not plan_of(c).wide:
        assert not E.dy16_supported(c), what
        rc, _, msg = _launch16(E, c, inp, d16)
        assert rc != 0 and 'only for wide layers' in msg, '%s: dy16 on a narrow layer: %d %r' % (what, rc, msg)
        return
    assert c.kind == 'x' or E.dy16_supported(c), what

    def call():
        rc, o, msg = _launch16(E, c, inp, d16)
        assert rc == 0, (what, rc, msg)
        return (o,)
    got, = _twice(what + ' dy16', call, (ncol,))
    assert np.array_equal(np.ascontiguousarray(got[..., :ncol]).view(np.uint32), np.ascontiguousarray(one_pass[..., :ncol]).view(np.uint32)), \
        what + ': the dy16 entry differs from the fp32-dy entry at passes = 1'


def _forward(E, c, what, inp, passes, ref_pre=None):
    """The forward with the ReLU and its mask (twice) and without.  With ``ref_pre``: bit for bit against it.  Returns
    (out [B, Fout, M], the mask bytes, out without ReLU)."""
    M, Mq = c.M, (c.M + 3) // 4
    out, mask = _twice(what + ' fwd', lambda: _launch(E, c, inp, passes, 1), (M, Mq))
    out0 = inside(_launch(E, c, inp, passes, 0)[0], what)
    assert np.isfinite(out[..., :M]).all() and np.isfinite(out0[..., :M]).all(), what + ': a value that is not finite'
    assert np.array_equal(unpack_mask(mask, M), out[..., :M] > 0), what + ': the mask is not out > 0'
    if ref_pre is not None:
        _bits_equal(what + ' out', out[..., :M], out_ref(ref_pre, 1))
        _bits_equal(what + ' out without ReLU', out0[..., :M], ref_pre)
        assert np.array_equal(unpack_mask(mask, M), ref_pre > 0), what + ': the mask is not pre > 0'
    return out[..., :M], np.ascontiguousarray(mask), out0[..., :M]


def _round_trip(E, c, what, inp, mask):
    """chebgcn_relu_grad_bf16 on the forward's own mask: dy16 = RNE(mask ? dout : 0) bit for bit over [0, M)"""
    M = c.M
    d16, = _twice(what + ' relu_grad_bf16', lambda: (E.relu_grad16(c, inp.dout, mask),), (M,))
    want = bf16_bits(np.where(unpack_mask(mask, M), inp.dout[..., :M], np.float32(0)))
    assert np.array_equal(d16[..., :M], want), what + ': dy16 is not the RNE rounding of mask ? dout : 0'


def run_exact(E, c):
    """The exact leg of case ``c`` on the entries ``E``: every comparison bit for bit.  Returns the census."""
    assert_exact_arithmetic(c)
    ncol = None if c.kind == 'w' else c.M
    seen = {}
    for leg, all_passes in legs_of(c):
        for pad in PADS[leg]:
            what = '%s leg %s pad %s' % (case_id(c), leg, pad)
            inp = make_inputs(c, leg, pad)
            seen.update(('%s_%s' % (leg, k), v) for k, v in census(c, leg, inp, pad).items())
            for passes in all_passes:
                w = '%s P%d' % (what, passes)
                ref = exact_ref(c, leg, inp, passes)
                if c.kind == 'f':
                    _, mask, _ = _forward(E, c, w, inp, passes, ref)
                    if leg == 'a':
                        _round_trip(E, c, w, inp, mask)
                    continue
                got, = _twice(w, lambda: _launch(E, c, inp, passes), (ncol,))
                _bits_equal(w, got[..., :ncol], ref)
                if leg == 'a' and passes == 1:
                    _dy16_identity(E, c, w, inp, got)
    return seen


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def run_roundoff(E, c):
    """The emulated round-off leg: {name: (error against the emulation, its bound, error against the plain product, its bound)},
    both relative to the reference's max.  The bit-identities are asserted here, the bounds by ``assert_roundoff``."""
    what = case_id(c) + ' round-off'
    inp = make_inputs(c, 'r')
    full = plain(c, inp)
    ncol = None if c.kind == 'w' else c.M
    m = {}
    for passes in (1, 3):
        ref = EMU[c.kind](c, inp, passes)
        if c.kind == 'f':
            out, mask, out0 = _forward(E, c, '%s P%d' % (what, passes), inp, passes)
            scale = np.abs(ref).max()
            err = max(np.abs(out - out_ref(ref, 1)).max(), np.abs(out0 - ref).max()) / scale
            perr = max(np.abs(out - out_ref(full, 1)).max(), np.abs(out0 - full).max()) / np.abs(full).max()
            m['fwd P%d' % passes] = (float(err), REL, float(perr), BF16_REL if passes == 1 else SPLIT_REL)
            if passes == 1:
                _round_trip(E, c, what, inp, mask)
            continue
        got = inside(_launch(E, c, inp, passes)[0], what)
        assert np.isfinite(got[..., :ncol]).all(), '%s P%d: a value that is not finite' % (what, passes)
        g64 = got[..., :ncol].astype(np.float64)
        m['bwd_%s P%d' % (c.kind, passes)] = (_rel(g64, ref), GREL, _rel(g64, full), BF16_REL if passes == 1 else SPLIT_REL)
        if passes == 1:
            _dy16_identity(E, c, what, inp, got)
    for name, (err, bound, perr, pbound) in sorted(m.items()):
        print('%s %s: %.3e of the emulation (bound %.0e, %.3f of it), %.3e of the plain product (bound %.0e)' % (
            what, name, err, bound, err / bound, perr, pbound))
    return m


def assert_roundoff(c, m):
    for name, (err, bound, perr, pbound) in sorted(m.items()):
        assert err <= bound, '%s %s: %.3e of the emulated arithmetic, above %.0e' % (case_id(c), name, err, bound)
        assert perr <= pbound, '%s %s: %.3e of the plain product, above %.0e' % (case_id(c), name, perr, pbound)


# ------------------------------------------------------------------------------------------------------------ the device's entries

def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Device:
    """The C entries on padded host arrays: uploads (cached per array), guarded device outputs and workspaces, the dispatch
    assertion, and the outputs back on the host, guards included."""

    def __init__(self, lib):
        self.lib = lib
        self.held = {}

    def up(self, a):
        if a is None:
            return None
        if id(a) not in self.held:
            h = np.ascontiguousarray(a)
            self.held[id(a)] = (a, torch.from_numpy(h.view(np.int16) if h.dtype == U16 else h).to(DEV))
        return ctypes.c_void_p(self.held[id(a)][1].data_ptr())

    @staticmethod
    def buf(shape, dtype=np.float32):
        """(device tensor guards included, pointer to its inside, host Out to come back into)"""
        o, _ = new_out(shape, dtype)
        t = torch.from_numpy(o.whole.view(np.int16) if o.whole.dtype == U16 else o.whole).to(DEV)
        return t, ctypes.c_void_p(t.data_ptr() + GUARD * o.whole.itemsize), o

    @staticmethod
    def down(b):
        w = b[0].cpu().numpy()
        return T.Out(w.view(np.uint16) if b[2].whole.dtype == U16 else w, b[2].shape)

    def ran(self, c, rc, entry, want):
        _lib.check(rc, entry)
        got = _lib.last_dispatch()
        assert got == want, '%s %s: launched %r, predicted %r (%s)' % (case_id(c), entry, got, want, ASSUMES)
        torch.cuda.synchronize()

    def workspace(self, c, n, want):
        """exactly ``n`` bytes (the library's figure, which must be the restatement's) between sentinels, made on the device"""
        assert n == want, '%s: a workspace of %d bytes, the restatement says %d (%s)' % (case_id(c), n, want, ASSUMES)
        t = torch.full((n + 2 * GUARD,), T.SENT[np.dtype(np.uint8)], dtype=torch.uint8, device=DEV)
        t[GUARD:GUARD + n] = T.POISON[np.dtype(np.uint8)]
        return t, ctypes.c_void_p(t.data_ptr() + GUARD), n

    def ws_intact(self, c, ws):
        t, _, n = ws
        s = T.SENT[np.dtype(np.uint8)]
        assert bool((t[:GUARD] == s).all()) and bool((t[GUARD + n:] == s).all()), case_id(c) + ': a store left the workspace'

    def _bwd_w_ws(self, c):
        for k, v in knobs_of(c).items():
            assert os.environ.get(k) == v, '%s: %s is %r in the environment, the case needs %r' % (case_id(c), k, os.environ.get(k), v)
        n = self.lib.chebgcn_contract_bwd_w_bf16_workspace(c.B, c.M, c.Fin, c.K, c.Fout)
        return self.workspace(c, n, bwb_workspace(plan_of(c))), n

    def bwd_w(self, c, stack, dy, passes):
        dW = self.buf((c.Fin * c.K, c.Fout))
        ws, n = self._bwd_w_ws(c)
        rc = self.lib.chebgcn_contract_bwd_w_bf16(self.up(stack), self.up(dy), dW[1], ws[1], n, c.B, c.M, c.Fin, c.K, c.Fout, passes,
                                                  _stream())
        self.ran(c, rc, 'contract_bwd_w_bf16', bwd_w_arm(plan_of(c), passes))
        self.ws_intact(c, ws)
        return self.down(dW)

    def dy16_supported(self, c):
        return bool(self.lib.chebgcn_bf16_dy16_supported(c.B, c.M, c.Fin, c.K, c.Fout))

    def bwd_w_dy16(self, c, stack, d16):
        dW = self.buf((c.Fin * c.K, c.Fout))
        ws, n = self._bwd_w_ws(c)
        before = _lib.last_dispatch()
        rc = self.lib.chebgcn_contract_bwd_w_bf16_dy16(self.up(stack), self.up(d16), dW[1], ws[1], n, c.B, c.M, c.Fin, c.K, c.Fout,
                                                       _stream())
        if rc != 0:
            assert _lib.last_dispatch() == before, case_id(c) + ': a refused call enqueued ' + _lib.last_dispatch()
            return rc, None, (self.lib.chebgcn_last_error() or b'').decode()
        self.ran(c, rc, 'contract_bwd_w_bf16_dy16', bwd_w_arm(plan_of(c), 1, dy16=True))
        self.ws_intact(c, ws)
        return rc, self.down(dW), ''

    def _bwd_x(self, c, dy, W, passes, x16):
        gs = self.buf((c.K, c.B, c.Fin, plane_stride(c.M)))
        n = self.lib.chebgcn_contract_bwd_x_bf16_workspace(c.Fin, c.K, c.Fout)
        ws = self.workspace(c, n, bwd_x_workspace(c.Fin * c.K, c.Fout))
        if x16:
            rc = self.lib.chebgcn_contract_bwd_x_bf16_dy16(self.up(dy), self.up(W), gs[1], c.B, c.M, c.Fin, c.K, c.Fout, ws[1], n, _stream())
        else:
            rc = self.lib.chebgcn_contract_bwd_x_bf16(self.up(dy), self.up(W), gs[1], c.B, c.M, c.Fin, c.K, c.Fout, passes, ws[1], n,
                                                      _stream())
        self.ran(c, rc, 'contract_bwd_x_bf16' + ('_dy16' if x16 else ''), bwd_x_arm(c.Fin * c.K, passes, x16))
        self.ws_intact(c, ws)
        return self.down(gs)

    def bwd_x(self, c, dy, W, passes):
        return self._bwd_x(c, dy, W, passes, False)

    def bwd_x_dy16(self, c, d16, W):
        return self._bwd_x(c, d16, W, 1, True)

    def fwd(self, c, stack, W, bias, relu, passes):
        Mp = plane_stride(c.M)
        out = self.buf((c.B, c.Fout, Mp))
        mask = self.buf((c.B, c.Fout, Mp // 4), np.uint8) if relu else None
        n = self.lib.chebgcn_contract_fwd_bf16_workspace(c.Fin, c.K, c.Fout)
        ws = self.workspace(c, n, fwd_workspace(c.Fin * c.K, c.Fout))
        rc = self.lib.chebgcn_contract_fwd_bf16(self.up(stack), self.up(W), self.up(bias), c.bias, out[1], mask[1] if relu else None,
                                                c.B, c.M, c.Fin, c.K, c.Fout, 1, 0, relu, passes, ws[1], n, _stream())
        self.ran(c, rc, 'contract_fwd_bf16', fwd_arm(c.Fout, passes))
        self.ws_intact(c, ws)
        return self.down(out), self.down(mask) if relu else None

    def relu_grad16(self, c, dout, mask):
        d16 = self.buf((c.B, c.Fout, plane_stride(c.M)), np.uint16)
        rc = self.lib.chebgcn_relu_grad_bf16(self.up(dout), self.up(mask), d16[1], None, N, c.B, c.M, c.Fout, None, 0, _stream())
        self.ran(c, rc, 'relu_grad_bf16', relu_grad16_arm(c.M, c.Fout))
        return self.down(d16)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS, ASSUMES
    return _lib.lib()


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_exact_leg(lib, monkeypatch, c):
    """Operands whose sums are exact: every output of every entry bit for bit, twice (``run_exact``)."""
    set_knobs(monkeypatch, c)
    seen = run_exact(Device(lib), c)
    record_measured('contract_bf16_arms_exact[%s]' % case_id(c), **seen)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_roundoff_leg(lib, monkeypatch, c):
    """Standard-normal operands against the float64 sum of the emulated bf16 arithmetic: 1e-5 of max forward, 2e-5 of max for the
    gradients, one-pass arms included (``run_roundoff``)."""
    set_knobs(monkeypatch, c)
    m = run_roundoff(Device(lib), c)
    record_measured('contract_bf16_arms_roundoff[%s]' % case_id(c),
                    **{k.replace(' ', '_'): v[0] for k, v in m.items()},
                    **{k.replace(' ', '_') + '_plain': v[2] for k, v in m.items()},
                    worst_ratio=max(v[0] / v[1] for v in m.values()))
    assert_roundoff(c, m)


def test_tables_reach_every_arm():
    """The case table reaches every arm named in the module docstring, by the dispatch restatement (which every launch checks
    against chebgcn_last_dispatch())."""
    reach = table_reach()
    record_measured('contract_bf16_arms_tables', cases=len(CASES), **reach)
