#!/usr/bin/env python3
"""What the convolutive engine (nmfd_engine.ConvMU) decides and launches, recorded without a GPU.

    python tools/make_golden_conv_plan.py [--out tests/golden/g22_conv_plan.npz]

Two recordings of the tree the tool runs in (libnmfmu.so built; its static predicates run on the host):

* plan grid: ConvMU constructed on ``device='meta'`` tensors (CPU tensors for precision='auto', which looks at data) over
  points() -- shapes, beta, precision, own_loop, CU count and the TORCHNMF_AMD_NMFD_* switches.  The outcome of a point is every
  decision the constructor left on the engine (FIELDS), the element count of every buffer it allocated, whether it warned,
  or the type of the exception it raised.
* launch trace: for every case of tests/conv_emulation.conv_cases() the engine runs on CPU tensors behind a proxy of the
  library that logs every call that would launch (symbol, scalars, nmfmu_gemm_desc fields, pointers as buffer name + byte
  offset) and answers 0; the host-side queries (HOST_CALLS) pass through.

The fixture holds the table of distinct outcome strings and id arrays.  It is recorded from the tree BEFORE a change of the
engine's host side (the parent commit, e.g. a `git worktree` with its library built); tests/test_conv_plan_trace.py walks the
same points on the working tree and requires equal outcomes.  A pull request that changes a decision on purpose re-records
the fixture and reviews the difference this tool prints against the old one.
"""
import argparse
import contextlib
import ctypes as C
import itertools
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g22_conv_plan.npz')
for _p in (os.path.join(ROOT, 'pytorch-nmf_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from torchnmf_amd import _capi, nmfd_engine as N  # noqa: E402

PREFIX = 'TORCHNMF_AMD_NMFD_'
# the 13 switches of the engine with their non-default value
SWITCHES = {'WINSTAGE': '0', 'EXPLICIT': '1', 'FOLD_PARTS': '0', 'FUSED_SUMS': '0', 'FUSED_TABLES': '0', 'H_ROWS': '0',
            'H_FOLD': '0', 'KSPLIT': '0', 'ROWS_FUSED': '0', 'TAIL_SPLIT': '0', 'RAGGED': '0', 'RAGGED_IN_GRID': '0', 'NARROW': '0'}
# what the constructor decides, as plain attributes of the engine (None: the path that owns the attribute was not taken)
FIELDS = ('precision_name', 'L', 'T', 'Lh', 'c_pad', 'bl_pad', 'rp_pad', 'implicit', 'fold_parts', 'h_rows', 'ragged',
          'ragged_in_grid', 'c_main', 'c_rows', 'fused_sums', 'fused_tables', 'rows_fused', 'h_tail_rows', 'h_tail_split',
          'wk_rows', 'wk_fold', 'wk_klen', 'hj_pad', 'h_ksplit', 'w_ksplit', 'n_hparts', 'stage_mode', 'loss_main')
# the calls that launch nothing (host-side predicates and queries): they reach the real library
HOST_CALLS = ('nmfmu_fold_parts_supported', 'nmfmu_conv_table_bytes', 'nmfmu_convnd_table_bytes', 'nmfmu_conv_ragged_supported',
              'nmfmu_gemm_ragged_supported', 'nmfmu_conv_ragged_blocks', 'nmfmu_fold_part_bytes', 'nmfmu_fold_hsum_parts',
              'nmfmu_fold_hsum_parts_tables', 'nmfmu_conv_h_rows_parts', 'nmfmu_convnd_koff', 'nmfmu_gemm_window_staged')


# ---- the grid -----------------------------------------------------------------------------------------------------------
def _up8(n):
    return (n + 7) // 8 * 8


TAPS = (1, 2, 7, 8, 9, 16, 63, 64, 65, 72, 127, 128, 129, 136)
CHANNELS = (63, 64, 65, 127, 128, 129, 136, 137, 1023, 1024, 1025, 1032, 1033)
RANKS = (31, 32, 33, 63, 64, 65, 255, 256, 257)
PRECISIONS = ('auto', 'bf16', 'bf16x3', 'f16', 'f16r', 'f16x', 'fp8')     # the last is no precision
CUS = (64, 256, 304)
CONFIGS3 = (1, 1025, (8192,), 8, (400,))          # the NMFD benchmark
NMF2D = (1, 64, (256, 512), 8, (8, 16))           # the NMF2D benchmark
# (B, C, ls, R, ts): one or more shapes on every path -- explicit / implicit operands, store-then-fold, window operand with
# tap folds 1 / 2 / 4 and a split contraction, fold-parts with and without a tail round, ragged channels beside and inside
# the grid, the 64-row channel tile, two and three shift axes, T = 1 (ranks above 256)
SHAPES = (
    (2, 70, (61,), 6, (5,)), (1, 130, (203,), 3, (16,)), (1, 90, (150,), 300, (1,)), (2, 70, (200,), 5, (24,)),
    (1, 140, (256,), 8, (72,)), (2, 70, (256,), 2, (128,)), (1, 129, (264,), 3, (136,)), (1, 40, (640,), 2, (400,)),
    (2, 70, (1024,), 2, (128,)), (1, 200, (128,), 6, (16,)), (1, 100, (128,), 11, (64,)), (2, 70, (96,), 40, (8,)),
    (1, 136, (136,), 3, (16,)), (1, 1025, (1024,), 2, (128,)), (1, 1025, (1029,), 2, (128,)), (1, 2048, (2048,), 8, (128,)),
    (1, 1024, (1024,), 16, (64,)), (1, 1100, (1100,), 8, (129,)), CONFIGS3, NMF2D,
    (2, 20, (30, 40), 3, (8, 8)), (1, 70, (18, 24), 5, (3, 8)), (1, 20, (14, 19), 3, (3, 4)), (1, 64, (40, 1024), 4, (4, 64)),
    (1, 20, (6, 9, 16), 3, (2, 3, 8)), (1, 65, (6, 9, 16), 40, (2, 3, 8)), (1, 1024, (4, 16, 32), 8, (2, 4, 16)),
)
# window tables on both sides of 2 GiB (the GEMM lanes address them with 32-bit byte offsets): one shift axis (16 B R
# (Lh + T - 1 rounded) bytes and the like: the library's own figure decides) and several
BIG = (
    (1, 64, (524288 - 512,), 256, (8,)), (1, 64, (524288 + 512,), 256, (8,)), (2, 64, (262144,), 255, (16,)),
    (2, 64, (262144 + 1024,), 257, (16,)),
    (1, 64, (4096, 4096), 8, (8, 8)), (1, 64, (4096, 4096), 4, (8, 8)), (1, 64, (64, 512, 512), 8, (2, 2, 8)),
    (1, 64, (64, 512, 512), 3, (2, 2, 8)),
)


def _point(shape, beta=1.0, precision='bf16x3', own_loop=True, ncu=256, env=()):
    return shape + (float(beta), precision, own_loop, ncu, tuple(sorted(dict(env).items())))


def points():
    """The grid points (B, C, ls, R, ts, beta, precision, own_loop, ncu, env) in enumeration order."""
    out = []
    # one shift axis: taps x frames (aligned, not aligned, short) x rank at three channel counts; channels at five tap counts
    for T, R, Cc in itertools.product(TAPS, RANKS, (64, 129, 1025)):
        for L in (_up8(T + 130), _up8(T + 130) + 3, T + 20):
            out.append(_point((1, Cc, (L,), R, (T,))))
    for T, Cc, R, B in itertools.product((8, 16, 64, 128, 136), CHANNELS, (8, 64), (1, 2)):
        for L in (_up8(T + 1030), _up8(T + 130) + 3):
            out.append(_point((B, Cc, (L,), R, (T,)), precision='auto'))
    # two and three shift axes: taps of the last axis, channels around the 64-row tile, rank around the tap folds
    for tl, Cc, R, B in itertools.product((1, 7, 8, 16, 64), (63, 64, 65), (4, 8, 9, 33), (1, 2)):
        out.append(_point((B, Cc, (20, _up8(tl + 40)), R, (3, tl))))
        out.append(_point((B, Cc, (20, _up8(tl + 40) + 1), R, (3, tl))))
        out.append(_point((B, Cc, (5, 6, _up8(tl + 24)), R, (2, 3, tl)), beta=0.5))
    # modes: batch, beta, precision, own_loop at one CU count; the CU counts apart
    for s, beta, prec, own in itertools.product(SHAPES + BIG, (1.0, 0.5), PRECISIONS, (True, False)):
        out.append(_point(s, beta, prec, own))
        if s[0] == 1 and prec in ('auto', 'f16'):
            out.append(_point((2,) + s[1:], beta, prec, own))
    for s, beta, own, ncu in itertools.product(SHAPES, (1.0, 2.0), (True, False), CUS):
        out.append(_point(s, beta, 'bf16x3', own, ncu))
    # switches: each singly, the pairs that interact, a forced tail-round split
    envs = [{k: v} for k, v in SWITCHES.items()]
    envs.append({'FOLD_PARTS': '0', 'H_ROWS': '0'})
    envs += [{'EXPLICIT': '1', k: v} for k, v in SWITCHES.items() if k != 'EXPLICIT']
    envs += [{'TAIL_SPLIT': '2,2'}, {'TAIL_SPLIT': '1,3'}, {'TAIL_SPLIT': '1,6', 'KSPLIT': '0'}]
    for env, s, (beta, prec) in itertools.product(envs, SHAPES, ((1.0, 'bf16x3'), (1.0, 'auto'), (1.0, 'f16'), (0.5, 'bf16'))):
        out.append(_point(s, beta, prec, env=env))
    for env, s in itertools.product(envs[:14], BIG):
        out.append(_point(s, 1.0, 'f16', env=env))
    return out


# 'auto' looks at data: small CPU tensors at three magnitudes on shapes on both sides of F16_MIN_DIM
AUTO_SHAPES = ((1, 1024, (1024,), 8, (128,)), (1, 1023, (1024,), 8, (128,)), (1, 1024, (1024,), 7, (128,)),
               (1, 64, (1024,), 16, (64,)), (1, 64, (1016,), 16, (64,)), (1, 16, (32, 32), 16, (8, 8)),
               (1, 16, (32, 32), 15, (8, 8)), (1, 1024, (1029,), 8, (128,)))
AUTO_DATA = ('in_range', 'max_above_3e4', 'mean_below_2^-10')


def auto_points():
    out = []
    for s, data, env in itertools.product(AUTO_SHAPES, AUTO_DATA, ((), (('TORCHNMF_AMD_AUTO_F16', '0'),))):
        out.append((s, data, env))
    return out


# ---- running the engine without a GPU ----------------------------------------------------------------------------------
class _Props:
    def __init__(self, ncu):
        self.multi_processor_count = ncu


@contextlib.contextmanager
def no_gpu(ncu, env, lib=None):
    """The engine's few touches of the device stubbed: a ROCm device 'is there' with ``ncu`` CUs, the stream is 0, the
    environment holds the given switches alone, and (``lib``) a stand-in for the library."""
    saved_env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith('TORCHNMF_AMD_')}
    os.environ.update({(k if k.startswith('TORCHNMF_AMD_') else PREFIX + k): v for k, v in dict(env).items()})
    saved = (torch.cuda.is_available, torch.cuda.get_device_properties, N._stream, _capi.load)
    torch.cuda.is_available = lambda: True
    torch.cuda.get_device_properties = lambda *a, **k: _Props(ncu)
    N._stream = lambda: 0
    if lib is not None:
        _capi.load = lambda: lib
    try:
        yield
    finally:
        torch.cuda.is_available, torch.cuda.get_device_properties, N._stream, _capi.load = saved
        for k in [k for k in os.environ if k.startswith('TORCHNMF_AMD_')]:
            del os.environ[k]
        os.environ.update(saved_env)


@contextlib.contextmanager
def no_launches():
    """The three constructor steps that launch (packing the target, the first images) stubbed out: plan grid only."""
    saved = (N.ConvMU._pack2d, N.ConvMU._pack_w, N.ConvMU.refresh_images)
    N.ConvMU._pack2d = N.ConvMU._pack_w = N.ConvMU.refresh_images = lambda self, *a, **k: None
    try:
        yield
    finally:
        N.ConvMU._pack2d, N.ConvMU._pack_w, N.ConvMU.refresh_images = saved


def _buffers(eng):
    """{name: tensor} of every buffer the engine holds (plane sets as name.hi / name.lo, lists and dicts by index)."""
    out = {}

    def add(name, v):
        if isinstance(v, torch.Tensor):
            out[name] = v
        elif isinstance(v, (N._Planes, N._Table)):
            add(name + '.hi', v.hi)
            add(name + '.lo', v.lo)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                add(f'{name}[{i}]', x)
        elif isinstance(v, dict):
            for k, x in v.items():
                add(f'{name}[{k}]', x)
    for name, v in sorted(vars(eng).items()):
        if name not in ('_ck',):
            add(name, v)
    return out


def outcome(eng, warned):
    # (with a leading underscore: the name of stage_mode and loss_main before the plan existed)
    fields = tuple((f, getattr(eng, f, getattr(eng, '_' + f, None))) for f in FIELDS)
    sizes = tuple((k, v.numel()) for k, v in _buffers(eng).items())
    return repr((fields, ('warned', warned), sizes))


def _build(shape, beta, precision, own_loop, dev, data='in_range'):
    B, Cc, ls, R, ts = shape
    lhs = tuple(l - t + 1 for l, t in zip(ls, ts))
    if dev == 'meta':
        V, W, H = (torch.empty(s, device='meta') for s in ((B, Cc) + ls, (Cc, R) + ts, (B, R) + lhs))
    else:
        g = torch.Generator().manual_seed(7)
        V = torch.rand((B, Cc) + ls, generator=g) + 1e-3
        W = torch.rand((Cc, R) + ts, generator=g) + 1e-3
        H = torch.rand((B, R) + lhs, generator=g) + 1e-3
        if data == 'max_above_3e4':
            V[0, 0].reshape(-1)[0] = 3.1e4
        elif data == 'mean_below_2^-10':
            H.mul_(2.0 ** -10)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        eng = N.ConvMU(V, W, H, beta, precision=precision, own_loop=own_loop)
    return eng, bool(w)


def plan_outcome(pt):
    """Outcome string of one grid point: the engine on meta tensors, nothing launched."""
    *shape, beta, precision, own_loop, ncu, env = pt
    with no_gpu(ncu, env), no_launches():
        try:
            return outcome(*_build(tuple(shape), beta, precision, own_loop, 'meta'))
        except Exception as e:          # (the exception type is the outcome: the texts are the engine's to word)
            return type(e).__name__


def auto_outcome(pt):
    shape, data, env = pt
    with no_gpu(256, env), no_launches():
        try:
            return outcome(*_build(shape, 1.0, 'auto', True, 'cpu', data))
        except Exception as e:
            return type(e).__name__


# ---- launch trace ---------------------------------------------------------------------------------------------------------
class _Ptr(int):
    """An address in a logged call, named once the engine's buffers are known."""


class Recorder:
    """Stands in front of the library: HOST_CALLS reach it, every other call is logged and answers 0."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    @staticmethod
    def _desc(d):
        out = []
        for name, typ in d._fields_:
            v = getattr(d, name)
            out.append((name, _Ptr(v or 0) if typ is C.c_void_p else tuple(v) if hasattr(v, '__len__') else v))
        return tuple(out)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in HOST_CALLS:
            return fn
        types = _capi.SIGNATURES[name][1]

        def call(*args):
            rec = []
            for a, typ in zip(args[:-1], types):            # (the last argument is the stream)
                if typ is C.c_void_p:
                    rec.append(_Ptr(a or 0))
                elif hasattr(a, '_obj'):                    # byref(nmfmu_gemm_desc)
                    rec.append(self._desc(a._obj))
                elif isinstance(a, C.Array):
                    rec.append(tuple(a))
                else:
                    rec.append(a)
            self.calls.append((name, tuple(rec)))
            return 0
        return call

    def lines(self, eng):
        """The log with every address as 'buffer+byte offset' of the engine's buffers (W and H among them), None for a
        null pointer, '?' for anything else (the caller's V)."""
        spans = [(t.data_ptr(), t.numel() * t.element_size(), name) for name, t in _buffers(eng).items() if t.numel()]

        def name(v):
            if isinstance(v, _Ptr):
                return None if not v else next((f'{n}+{v - lo}' for lo, size, n in spans if lo <= v < lo + size), '?')
            return tuple(name(x) for x in v) if isinstance(v, tuple) else v
        return [repr(name(c)) for c in self.calls]


def launch_trace(case, own_loop=True):
    """Log lines of: construction, two w_step / h_step pairs, _loss_device, refresh_images, one more h_step (own_loop=False:
    construction alone, as the trainer and the PLCA state build it)."""
    import conv_emulation as CE
    rec = Recorder(_capi.load())
    V, W0, H0 = CE.make_problem(case)
    with no_gpu(256, case['env'], lib=rec):
        try:
            if case['wide'] and own_loop:
                eng = N.WideRankMU(V[0].t().contiguous(), W0[:, :, 0].contiguous(), H0[0].t().contiguous(), case['beta'],
                                   *case['regs'], precision=case['precision'])
                inner = eng.eng
            else:
                eng = inner = N.ConvMU(V, W0, H0, case['beta'], *case['regs'], precision=case['precision'], own_loop=own_loop)
            if own_loop:
                for _ in range(2):
                    eng.w_step()
                    eng.h_step()
                inner._loss_device()
                eng.refresh_images()
                eng.h_step()
        except Exception as e:
            return [type(e).__name__]
    return rec.lines(inner) + [repr(('staged', tuple(sorted(inner.staged.items())))), outcome(inner, False)]


def trace_points():
    import conv_emulation as CE
    cases = CE.conv_cases()
    return [(c, True) for c in cases] + [(c, False) for c in cases if not c['wide']]


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def walk():
    """(outcome strings, labels) of the tree this runs in, in enumeration order: plan grid, 'auto' on data, then the log
    lines of every launch trace, each trace closed by an 'end' line."""
    out, labels = [], []
    for pt in points():
        out.append(plan_outcome(pt))
        labels.append(('plan', pt))
    for pt in auto_points():
        out.append(auto_outcome(pt))
        labels.append(('auto', pt))
    for case, own in trace_points():
        log = launch_trace(case, own) + ['end']
        out += log
        labels += [('trace', case['id'], own, i) for i in range(len(log))]
    return out, labels


def save(path, trace):
    got, _ = trace
    table = sorted(set(got))
    index = {s: i for i, s in enumerate(table)}
    np.savez_compressed(path, outcomes=np.frombuffer('\0'.join(table).encode(), dtype=np.uint8),
                        ids=np.asarray([index[s] for s in got], dtype=np.min_scalar_type(len(table))),
                        n_plan=np.asarray([len(points()), len(auto_points()), len(trace_points())]))


def load_fixture(path=FIXTURE):
    z = np.load(path)
    if list(z['n_plan']) != [len(points()), len(auto_points()), len(trace_points())]:
        raise ValueError(f'{path}: the grid differs from tools/make_golden_conv_plan.py; re-record the fixture')
    return z['outcomes'].tobytes().decode().split('\0'), z['ids']


def _first_field(a, b):
    """The first differing field of two outcome strings (plan outcomes are reprs of nested tuples)."""
    try:
        ta, tb = eval(a, {}), eval(b, {})          # noqa: S307 -- reprs this tool wrote
        flat = lambda t: list(t[0]) + [t[1]] + list(t[2])
        for (ka, va), (kb, vb) in zip(flat(ta), flat(tb)):
            if (ka, va) != (kb, vb):
                return f'{ka}: fixture {va!r}, now {vb!r}' if ka == kb else f'fixture {ka}={va!r}, now {kb}={vb!r}'
    except Exception:
        pass
    return ''


def difference(table, want_ids, trace, limit=5):
    """'' when walk()'s result equals the fixture, else a report of the first differing points (case and field)."""
    got, labels = trace
    plan_n = len(points()) + len(auto_points())
    if got[:plan_n] and len(want_ids) >= plan_n:
        bad = [i for i in range(plan_n) if got[i] != table[want_ids[i]]]
    else:
        bad = []
    if not bad and len(got) != len(want_ids):
        bad = [next((i for i, (s, j) in enumerate(zip(got, want_ids)) if s != table[j]), min(len(got), len(want_ids)) - 1)]
        head = f'{len(got)} outcomes, the fixture has {len(want_ids)}: a launch trace changed its length; the first difference:'
    else:
        bad = bad or [i for i, (s, j) in enumerate(zip(got, want_ids)) if s != table[j]]
        if not bad:
            return ''
        head = f'{len(bad)} of {len(got)} outcomes differ; the first {min(limit, len(bad))}:'
    rep = [head]
    for i in bad[:limit]:
        want = table[want_ids[i]]
        rep.append(f'--- {labels[i]}\n{_first_field(want, got[i])}\nfixture: {want}\nnow:     {got[i]}')
    return '\n'.join(rep)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=FIXTURE)
    args = ap.parse_args()
    trace = walk()
    if os.path.exists(args.out):
        try:
            table, ids = load_fixture(args.out)
            print(f'against the existing {args.out}: ' + (difference(table, ids, trace) or 'no difference'))
        except (ValueError, KeyError) as e:
            print(f'existing fixture not comparable: {e}')
    save(args.out, trace)
    n = (len(points()), len(auto_points()), len(trace_points()))
    print(f'wrote {args.out}: {os.path.getsize(args.out)} bytes; plan points, auto points, traces: {n}; '
          f'{len(set(trace[0]))} distinct outcomes of {len(trace[0])}')


if __name__ == '__main__':
    sys.exit(main())
