#!/usr/bin/env python3
"""Dispatch trace of the dense-MU C ABI: what csrc/nmfmu_capi.hip launches for a half-step, read without a GPU.

    python tools/make_golden_dispatch.py --csrc DIR [--out tests/golden/g21_dispatch.npz]

Compiles DIR/nmfmu_capi.hip with the Makefile's flags, links it against tests/dispatch_trace_stubs.hip (launchers that log
their arguments instead of launching) and calls the entries of include/nmfmu.h over a grid of nmfmu_step structs whose
pointers are distinct fake addresses inside one buffer (never dereferenced).  The outcome of a call is its return code plus
the log lines of the launches it made.  The fixture holds the grid axes, the table of distinct outcome strings and, per build
of nmfmu_capi.hip (BUILDS), the outcome ids in enumeration order; tests/test_dispatch_trace.py walks the same grid on the
working tree and requires equal ids.

The fixture is recorded from the tree BEFORE a change (the parent commit's csrc, e.g. a `git worktree`); the code under test
never writes it.  A pull request that changes dispatch on purpose re-records it from its own tree and reviews the difference
this tool prints against the old fixture (--out names an existing file: the first differing grid points with both outcomes).

The grid is not the full product of its axes (that would be 5 million calls and a fixture of many MiB).  Kernel selection
(padded rank x precision x beta x block rows x stage) is walked completely at both contraction splits; the size axes and the
pointer variants are each crossed with the selections on which they can act (GRID below), every entry at every point.
"""
import argparse
import ctypes as C
import importlib.util
import itertools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, 'tests', 'dispatch_trace_stubs.hip')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g21_dispatch.npz')
HIPCC = os.environ.get('HIPCC') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc'))

_spec = importlib.util.spec_from_file_location('_nmfmu_capi_binding',
                                               os.path.join(ROOT, 'pytorch-nmf_amd', 'torchnmf_amd', '_capi.py'))
_capi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_capi)

# builds of nmfmu_capi.hip, each with its own id array in the fixture
BUILDS = {'default': [], 'sp_off': ['-DNMFMU_SP=0'], 'sp2_off': ['-DNMFMU_SP2=0'], 'debug_hooks': ['-DNMFMU_DEBUG_HOOKS']}

R_PADS = (32, 64, 128, 256)
PRECISIONS = (0, 1, 2, 3, 4, 5)                 # the five NMFMU_PREC_* and one that is none
BETAS = (1.0, 2.0, 0.0, 0.5, 1.5, 0.7)
BLOCK_ROWS = (128, 256, 64)                     # 64: invalid
STAGES = (0, 1, 2, 3, 4, 5, 6)
NSPLITS = (1, 3)
PANEL_ROWS = (1280, 1024, 256)                  # 20 tiles (20 / 3 -> 7 -> 8: both the x2 and the x4 rounding), 16, 4
OWNER_ROWS = (300, 4096)
VARIANTS = ('all', 'owner_p2_null', 'owner_colsum_part_null', 'slab_den_null', 'lo_null', 'stamps', 'loss_part_null')
NUM_CUS = (256, 304)
AXES = {'r_pad': R_PADS, 'precision': PRECISIONS, 'beta': BETAS, 'block_rows': BLOCK_ROWS, 'stage': STAGES, 'nsplit': NSPLITS,
        'panel_rows': PANEL_ROWS, 'owner_rows': OWNER_ROWS, 'num_cu': NUM_CUS}
# (r_pads, precisions, betas, block_rows, stages, nsplits, panel_rows, owner_rows, variants, rank or None = r_pad - 28)
_SOME_BETAS, _LIVE_STAGES = (1.0, 2.0, 0.5), (1, 3, 4, 5, 6)
GRID = (
    # kernel selection, complete
    (R_PADS, PRECISIONS, BETAS, BLOCK_ROWS, STAGES, NSPLITS, (1280,), (300,), ('all',), None),
    # sizes: grid, tiles per split and its rounding, partial counts
    (R_PADS, PRECISIONS, _SOME_BETAS, (128, 256), _LIVE_STAGES, NSPLITS, PANEL_ROWS, OWNER_ROWS, ('all',), None),
    # pointers: what is required, what decides the fused apply, what is dropped
    (R_PADS, PRECISIONS, _SOME_BETAS, (128, 256), _LIVE_STAGES, NSPLITS, (1280,), (300,), VARIANTS[1:], None),
    # r_pad != pad_rank(rank)
    ((64,), PRECISIONS, (1.0, 2.0), (128, 256), (1,), (1,), (1280,), (300,), ('all',), 20),
)
ENTRIES = ('mu_partial', 'den_partial', 'mu_step0', 'mu_step1', 'mu_step2', 'mu_apply', 'mu_apply_reduced', 'trainer_apply',
           'xb_partial', 'xb_step0', 'xb_step1', 'xb_step2', 'loss', 'loss_checkpoint', 'mu_step_with_loss', 'slab_reduce',
           'colsum_nparts', 'riding_loss_supported', 'riding_loss_part_count')

_FAKE = ('xp', 'o_f', 'o_p1_hi', 'o_p1_lo', 'o_p2_hi', 'o_p2_lo', 'o_colsum', 'o_colsum_part', 'p_f', 'p_p1_hi', 'p_p1_lo',
         'p_p2_hi', 'p_p2_lo', 'p_colsum', 'p_colsum_part', 'slab_num', 'slab_den', 'status', 'stamps', 'kl_den', 'loss_part',
         'out', 'num', 'den', 'grad', 'g_hi', 'g_lo', 'g_scale', 'fa', 'fa_snap', 'fb', 'fb_snap', 'tsums', 'stream', 'debug')


def compile_lib(csrc, extra, workdir, tag):
    """hipcc with the Makefile's FLAGS (+ extra) for nmfmu_capi.hip, the stub unit (against the headers of the same tree) once
    per workdir, one shared library."""
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^FLAGS\s*=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').replace('$(EXTRA)', '').split()
    stub_o = os.path.join(workdir, 'stubs.o')
    if not os.path.exists(stub_o):
        include = ['-I', csrc, '-I', os.path.join(csrc, '..', '..', 'include')]
        subprocess.run([HIPCC] + flags + include + ['-c', STUBS, '-o', stub_o], check=True)
    capi_o, lib = os.path.join(workdir, f'capi_{tag}.o'), os.path.join(workdir, f'libdispatch_{tag}.so')
    subprocess.run([HIPCC] + flags + list(extra) + ['-c', os.path.join(csrc, 'nmfmu_capi.hip'), '-o', capi_o], check=True)
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', capi_o, stub_o, '-o', lib], check=True)
    return lib


def load(path):
    lib = C.CDLL(path)
    for name, (res, args) in _capi.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    lib.nmfmu_trace_take.restype, lib.nmfmu_trace_take.argtypes = C.c_char_p, [C.c_void_p]
    return lib


def points():
    for block in GRID:
        *axes, rank = block
        for p in itertools.product(*axes):
            yield p + (rank,)


def walk(lib):
    """Outcome strings in enumeration order: the static queries, then every entry at every grid point."""
    buf = C.create_string_buffer(4096 * (len(_FAKE) + 2))
    base = C.addressof(buf)
    A = {n: base + 4096 * (i + 1) for i, n in enumerate(_FAKE)}
    out, labels = [], []
    lib.nmfmu_trace_take(base)

    def q(name, *args):
        out.append(str(getattr(lib, name)(*args)))
        labels.append((name,) + args)
    q('nmfmu_debug_set_buffer', A['debug'])      # (diagnostic builds: the stamp buffer then shows in FusedArgs.debug)
    pads = (0, 512, 4096)
    for r in R_PADS + (48,):
        for prec in PRECISIONS:
            q('nmfmu_supported', r, prec)
            for beta in BETAS:
                for name in ('nmfmu_block_rows', 'nmfmu_kernel_family', 'nmfmu_pp_lds_transpose_supported', 'nmfmu_xb_supported'):
                    q(name, r, prec, beta)
                for m, k in itertools.product(pads, (0,) + PANEL_ROWS):
                    q('nmfmu_step_block_rows', m, k, r, prec, beta, 256)
                    for br, ncu in itertools.product(BLOCK_ROWS, NUM_CUS):
                        q('nmfmu_choose_nsplit_for', m, k, r, prec, beta, br, ncu)
    for m, k, br, ncu in itertools.product(pads, (0,) + PANEL_ROWS, BLOCK_ROWS, NUM_CUS):
        q('nmfmu_choose_nsplit', m, k, br, ncu)
    for m, br, ns in itertools.product(pads, BLOCK_ROWS, NSPLITS):
        q('nmfmu_loss_part_count', m, br, ns)

    pad = lambda n: (n + 255) // 256 * 256
    s = A['stream']
    for pt in points():
        r_pad, prec, beta, br, stage, nsplit, k_rows, m_rows, var, rank = pt
        lo = var != 'lo_null'
        owner = _capi.Factor(A['o_f'], A['o_p1_hi'], A['o_p1_lo'] if lo else None, None if var == 'owner_p2_null' else A['o_p2_hi'],
                             A['o_p2_lo'] if lo else None, A['o_colsum'],
                             None if var == 'owner_colsum_part_null' else A['o_colsum_part'], m_rows, pad(m_rows))
        panel = _capi.Factor(A['p_f'], A['p_p1_hi'], A['p_p1_lo'] if lo else None, A['p_p2_hi'], A['p_p2_lo'] if lo else None,
                             A['p_colsum'], A['p_colsum_part'], k_rows, pad(k_rows))
        st = _capi.Step(A['xp'], owner, panel, A['slab_num'], None if var == 'slab_den_null' else A['slab_den'],
                        rank if rank is not None else r_pad - 28, r_pad, nsplit, prec, stage, br, beta, 0.75, 0.125, 0.25, A['status'],
                        A['stamps'] if var == 'stamps' else None)
        ref = C.byref(st)
        kl_den = A['kl_den'] if beta == 1.0 else None
        part = None if var == 'loss_part_null' else A['loss_part']
        gram = (A['g_hi'], A['g_lo'], A['g_scale'])
        calls = (
            lambda: lib.nmfmu_mu_partial(ref, s), lambda: lib.nmfmu_den_partial(ref, s),
            lambda: lib.nmfmu_mu_step(ref, kl_den, 0, s), lambda: lib.nmfmu_mu_step(ref, kl_den, 1, s),
            lambda: lib.nmfmu_mu_step(ref, kl_den, 2, s),
            lambda: lib.nmfmu_mu_apply(ref, None, None, 0, kl_den, s),
            lambda: lib.nmfmu_mu_apply(ref, A['num'], None if kl_den else A['den'], 1, kl_den, s),
            lambda: lib.nmfmu_trainer_apply(ref, None, None, 0, kl_den, 0.5, A['grad'], s),
            lambda: lib.nmfmu_xb_partial(ref, s), lambda: lib.nmfmu_xb_step(ref, *gram, 0, s),
            lambda: lib.nmfmu_xb_step(ref, *gram, 1, s), lambda: lib.nmfmu_xb_step(ref, *gram, 2, s),
            lambda: lib.nmfmu_loss(ref, part, A['out'], s),
            lambda: lib.nmfmu_loss_checkpoint(ref, part, A['out'], A['fa'], A['fa_snap'], 1024, A['fb'], A['fb_snap'], 2048, s),
            lambda: lib.nmfmu_mu_step_with_loss(ref, A['kl_den'], part, A['tsums'], A['out'], s),
            lambda: lib.nmfmu_slab_reduce(ref, A['num'], A['den'], s),
            lambda: lib.nmfmu_colsum_nparts(ref), lambda: lib.nmfmu_riding_loss_supported(ref),
            lambda: lib.nmfmu_riding_loss_part_count(ref),
        )
        for entry, call in zip(ENTRIES, calls):
            rc = call()
            out.append(f'{rc}\n{lib.nmfmu_trace_take(base).decode()}')
            labels.append((entry, pt))
    return out, labels


def describe(label):
    """A readable form of one label of walk()."""
    if label[0] in ENTRIES:
        names = ('r_pad', 'precision', 'beta', 'block_rows', 'stage', 'nsplit', 'panel_rows', 'owner_rows', 'pointers', 'rank')
        return f'{label[0]} at ' + ', '.join(f'{k}={v}' for k, v in zip(names, label[1]))
    return f'{label[0]}{label[1:]}'


def trace_builds(csrc, builds=BUILDS):
    """{build: (outcome strings, labels)} of DIR's nmfmu_capi.hip."""
    work = tempfile.mkdtemp(prefix='dispatch_trace_')
    try:
        return {tag: walk(load(compile_lib(csrc, builds[tag], work, tag))) for tag in builds}
    finally:
        shutil.rmtree(work, ignore_errors=True)


def save(path, traces):
    table = sorted(set(itertools.chain.from_iterable(tr for tr, _ in traces.values())))
    index = {s: i for i, s in enumerate(table)}
    arrays = {'axis_' + k: np.asarray(v, dtype=np.float64) for k, v in AXES.items()}
    arrays['variants'], arrays['entries'] = np.asarray(VARIANTS), np.asarray(ENTRIES)
    arrays['outcomes'] = np.frombuffer('\0'.join(table).encode(), dtype=np.uint8)      # the distinct strings, NUL-separated
    for tag, (tr, _) in traces.items():
        arrays['ids_' + tag] = np.asarray([index[s] for s in tr], dtype=np.min_scalar_type(len(table)))
    np.savez_compressed(path, **arrays)


def load_fixture(path=FIXTURE):
    """(outcome table, {build: ids}) of a fixture; raises when its axes are not this file's."""
    z = np.load(path)
    for k, v in AXES.items():
        if list(z['axis_' + k]) != [float(x) for x in v]:
            raise ValueError(f'{path}: axis {k} differs from tools/make_golden_dispatch.py; re-record the fixture')
    if list(z['variants']) != list(VARIANTS) or list(z['entries']) != list(ENTRIES):
        raise ValueError(f'{path}: pointer variants or entries differ from tools/make_golden_dispatch.py; re-record the fixture')
    table = z['outcomes'].tobytes().decode().split('\0')
    return table, {k[len('ids_'):]: z[k] for k in z.files if k.startswith('ids_')}


def difference(table, want_ids, trace, limit=5):
    """'' when the trace (walk's result) equals the fixture's ids, else a report of the first differing grid points."""
    got, labels = trace
    if len(got) != len(want_ids):
        return f'{len(got)} outcomes, the fixture has {len(want_ids)}: the grid changed; re-record the fixture'
    bad = [i for i, (s, j) in enumerate(zip(got, want_ids)) if s != table[j]]
    if not bad:
        return ''
    rep = [f'{len(bad)} of {len(got)} outcomes differ; the first {min(limit, len(bad))}:']
    for i in bad[:limit]:
        rep.append(f'--- {describe(labels[i])}\nfixture: {table[want_ids[i]]!r}\nnow:     {got[i]!r}')
    return '\n'.join(rep)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--csrc', required=True, help='directory of the nmfmu_capi.hip (and Makefile) to record')
    ap.add_argument('--out', default=FIXTURE)
    args = ap.parse_args()
    traces = trace_builds(os.path.abspath(args.csrc))
    if os.path.exists(args.out):
        try:
            table, ids = load_fixture(args.out)
            for tag, tr in traces.items():
                print(f'[{tag}] against the existing {args.out}: ' + (difference(table, ids[tag], tr) or 'no difference'))
        except (ValueError, KeyError) as e:
            print(f'existing fixture not comparable: {e}')
    save(args.out, traces)
    n = {tag: len(tr) for tag, (tr, _) in traces.items()}
    print(f'wrote {args.out}: {os.path.getsize(args.out)} bytes, outcomes per build {n}')


if __name__ == '__main__':
    sys.exit(main())
