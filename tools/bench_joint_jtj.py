"""Time one evaluation of the joint normal equations, ops.joint_jtj_jtr
(joint_jtj.hip) against reference.joint_jtj_jtr on the same device tensors,
and one lm.joint_lm_solve(maxiter=4) with SAGECAL_JOINT_KERNEL on and off.

    python tools/bench_joint_jtj.py --out profiles/joint_jtj.json

Shape a: 64 stations, 10 clusters, T = 60, one chunk per cluster, dense.
Shape b: the same with 16 chunks per cluster and T = 64 (60 timeslots leave
the 16th chunk empty), blocked; the torch path is tried once and reported as
not fitting when it runs out of memory. Device events around each call, the
two paths alternating; needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sagecal_amd.ops import dispatch as ops          # noqa: E402
from sagecal_amd.ops import reference as R           # noqa: E402
from sagecal_amd.solvers import lm                   # noqa: E402

DEV = 'cuda:0'


def make(N, M, T, K, seed=3):
    g = torch.Generator().manual_seed(seed)
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase = len(pairs)

    def cplx(*shape):
        return torch.randn(*shape, dtype=torch.complex64, generator=g).to(DEV)
    nchunks = [K] * M
    chunk_off = [ci * K for ci in range(M)]
    Jt = torch.eye(2, dtype=torch.complex64, device=DEV) \
        + 0.2 * cplx(M * K, N, 2, 2)
    cohs = cplx(M, T * Nbase, 2, 2)
    bb = torch.tensor(np.tile(pairs, (T, 1)), device=DEV)
    x = sum(R.apply_jones(cohs[ci], Jt[ci * K:(ci + 1) * K], bb,
                          R.chunk_rows_for(ci, nchunks, T, Nbase, T * Nbase,
                                           DEV)) for ci in range(M))
    x = x + 0.01 * cplx(T * Nbase, 2, 2)
    J = Jt + 0.05 * cplx(M * K, N, 2, 2)
    return x, cohs, J, chunk_off, nchunks, bb, T, Nbase


def time_ms(fn):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms):
    return {'ms_per_call': [round(v, 4) for v in ms],
            'ms_median': round(statistics.median(ms), 4),
            'ms_spread': round(max(ms) - min(ms), 4)}


def compare(fns, warmup, runs):
    """Alternate the callables of `fns` {name: fn}; per-name timings."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(time_ms(fn)[0])
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/joint_jtj.json')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    res = {'tool': 'tools/bench_joint_jtj.py', 'warmup': args.warmup,
           'runs': args.runs, 'order': 'kernel, torch, kernel, torch, ...',
           'device': 'MI355X (gfx950)', 'shapes': {}}

    a = make(64, 10, 60, 1)
    out = compare({'kernel': lambda: ops.joint_jtj_jtr(*a),
                   'torch': lambda: R.joint_jtj_jtr(*a)},
                  args.warmup, args.runs)
    Hk, gk, ck = ops.joint_jtj_jtr(*a)
    Ht, gt, ct = R.joint_jtj_jtr(*a)
    out['H_max_abs_diff_over_max_abs'] = float((Hk - Ht).abs().max()
                                               / Ht.abs().max())
    out['g_max_abs_diff_over_max_abs'] = float((gk - gt).abs().max()
                                               / gt.abs().max())
    out['cost_kernel_over_torch_minus_1'] = float(ck / ct - 1)
    out['torch_over_kernel'] = round(out['torch']['ms_median']
                                     / out['kernel']['ms_median'], 2)
    out['kernel_is_faster'] = bool(
        out['torch']['ms_median'] - out['kernel']['ms_median']
        > out['torch']['ms_spread'])
    del Hk, Ht
    solve = {}
    for name, flag in (('switch_on', '1'), ('switch_off', '0'),
                       ('switch_on', '1'), ('switch_off', '0')):
        os.environ['SAGECAL_JOINT_KERNEL'] = flag
        ms, (_, cost) = time_ms(lambda: lm.joint_lm_solve(*a, maxiter=4))
        solve.setdefault(name, []).append(
            {'ms': round(ms, 2), 'final_cost': cost})
    os.environ.pop('SAGECAL_JOINT_KERNEL')
    out['joint_lm_solve_maxiter4'] = dict(
        solve, note='two calls each, alternating; the first of each also '
        'builds its index tables')
    res['shapes']['a_dense_P5120'] = out

    b = make(64, 10, 64, 16)
    out = compare({'kernel': lambda: ops.joint_jtj_jtr(*b, blocked=True)},
                  args.warmup, args.runs)
    try:
        torch.cuda.reset_peak_memory_stats()
        ms = [time_ms(lambda: R.joint_jtj_jtr(*b)[2])[0] for _ in range(2)]
        out['torch_dense'] = dict(
            summary(ms), peak_bytes=torch.cuda.max_memory_allocated())
    except torch.OutOfMemoryError as e:
        out['torch_dense'] = f'does not fit: {str(e)[:120]}'
    res['shapes']['b_blocked_16x5120'] = out

    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
