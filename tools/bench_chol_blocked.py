"""Time the blocked Cholesky kernels (cholesky_blocked.hip) through
hip_host.chol_solve_damped with SAGECAL_CHOL_BLOCKED=1 against the path
lm._joint_lm_blocked takes without the switch, torch one block at a time
(lm._chol_solve), on the same device tensors [16, 5120, 5120] and
[1, 5120, 5120]; for information, ext.chol_solve_blocked against
ext.chol_solve_mw at [16, 4096, 4096]; and the error figures behind the
limit of tests/test_gpu_chol_blocked.py::test_above_the_old_limit, on that
test's inputs.

    python tools/bench_chol_blocked.py --out profiles/chol_blocked.json

Device events around each call, the two paths alternating, median of --runs
after --warmup; needs a GPU. Kernel durations come from a second run under
the profiler, which slows the host and so gets no timings of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/bench_chol_blocked.py --profile-run
    python tools/bench_chol_blocked.py --out profiles/chol_blocked.json \\
        --merge-kernels DIR/.../NAME_kernel_stats.csv

--profile-run solves [16, 5120, 5120] PROFILE_CALLS times and writes
nothing; --merge-kernels adds the per-kernel split and the update kernel's
achieved rates, from flops and bytes counted here from the shapes, to an
existing result file and needs no GPU."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sagecal_amd.ops import hip_host                 # noqa: E402
from sagecal_amd.solvers import lm                   # noqa: E402

DEV = 'cuda:0'
X = 128
PROFILE_CALLS = 3
SWITCH = 'SAGECAL_CHOL_BLOCKED'


def make(batch, n, seed=5):
    """A = G G^T / n + 0.5 I, b, mu in [0.01, 1), built on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.empty(batch, n, n, device=DEV)
    for k in range(batch):
        G = torch.randn(n, n, device=DEV, generator=g)
        A[k] = G @ G.T / n
    A.diagonal(dim1=1, dim2=2).add_(0.5)
    b = torch.randn(batch, n, device=DEV, generator=g)
    mu = 0.01 + 0.99 * torch.rand(batch, device=DEV, generator=g)
    return A, b, mu


def torch_blocks(A, b, mu):
    """The switch-off branch of lm._joint_lm_blocked; it damps A in place,
    so the diagonal is restored afterwards."""
    d = A.diagonal(dim1=-2, dim2=-1)
    d.add_(mu[:, None])
    dp = torch.stack([lm._chol_solve(A[k], b[k]) for k in range(A.shape[0])])
    d.sub_(mu[:, None])
    return dp


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
    """Alternate the callables of `fns` {name: fn}; per-name timings, and
    whether the first is faster than the second by more than its spread."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(time_ms(fn)[0])
    out = {k: summary(v) for k, v in ms.items()}
    new, old = list(fns)
    out[f'{old}_over_{new}'] = round(out[old]['ms_median']
                                     / out[new]['ms_median'], 2)
    out[f'{new}_is_faster'] = bool(
        out[old]['ms_median'] - out[new]['ms_median'] > out[old]['ms_spread'])
    return out


def rel(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).abs().max()
                 / ref.abs().max())


def syrk_counts(n, batch):
    """(flops, bytes) of all k_cholxl_syrk launches of one solve: per
    128x128 tile of the lower tile grid 2*128^3 flops (edge tiles counted
    by their live rows and columns), the tile of L read and written once and
    the two 128 x 128 operand panels read once (one on a diagonal tile is
    counted twice, as the kernel loads it)."""
    flops = nbytes = 0
    for k in range(0, n - X, X):
        t0 = k + X
        tc = -(-(n - t0) // X)
        for i in range(tc):
            ri = min(X, n - t0 - i * X)
            for j in range(i + 1):
                cj = min(X, n - t0 - j * X)
                flops += 2 * ri * cj * X
                nbytes += 4 * (2 * ri * cj + X * (ri + cj))
    return flops * batch, nbytes * batch


def merge_kernels(out, stats_csv):
    with open(out) as f:
        res = json.load(f)
    rows = {}
    with open(stats_csv, newline='') as f:
        for r in csv.DictReader(f):
            if r['Name'].startswith('k_chol'):
                rows[r['Name']] = {
                    'calls': int(r['Calls']),
                    'total_ms': round(int(r['TotalDurationNs']) / 1e6, 4),
                    'average_us': round(float(r['AverageNs']) / 1e3, 2)}
    total = sum(r['total_ms'] for r in rows.values())
    for r in rows.values():
        r['share'] = round(r['total_ms'] / total, 4)
    flops, nbytes = syrk_counts(5120, 16)
    s = rows['k_cholxl_syrk']['total_ms'] / PROFILE_CALLS / 1e3
    res['kernel_trace'] = {
        'what': f'--profile-run under rocprofv3 --kernel-trace --stats: '
                f'{PROFILE_CALLS} solves of [16, 5120, 5120]',
        'kernel_ms_per_solve': round(total / PROFILE_CALLS, 3),
        'kernels': rows,
        'k_cholxl_syrk_per_solve': {
            'flops_from_shapes': flops, 'bytes_from_shapes': nbytes,
            'tflops_achieved': round(flops / s / 1e12, 2),
            'gbytes_per_s_achieved': round(nbytes / s / 1e9, 1)}}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/chol_blocked.json')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--merge-kernels', metavar='CSV')
    args = ap.parse_args()
    if args.merge_kernels:
        return merge_kernels(args.out, args.merge_kernels)
    assert torch.cuda.is_available(), 'needs a GPU'
    os.environ[SWITCH] = '1'
    if args.profile_run:
        A, b, mu = make(16, 5120)
        for _ in range(PROFILE_CALLS):
            hip_host.chol_solve_damped(A, b, mu)
        torch.cuda.synchronize()
        return
    res = {'tool': 'tools/bench_chol_blocked.py', 'warmup': args.warmup,
           'runs': args.runs, 'order': 'blocked, other, blocked, other, ...',
           'device': 'MI355X (gfx950)', 'shapes': {}}
    for batch in (16, 1):
        A, b, mu = make(batch, 5120)
        out = compare(
            {'blocked': lambda: hip_host.chol_solve_damped(A, b, mu),
             'torch_blocks': lambda: torch_blocks(A, b, mu)},
            args.warmup, args.runs)
        out['dp_max_abs_diff_over_max_abs'] = rel(
            hip_host.chol_solve_damped(A, b, mu), torch_blocks(A, b, mu))
        res['shapes'][f'{batch}x5120'] = out
        del A
    A, b, mu = make(16, 4096)
    ext = hip_host._ext()
    sc = torch.empty(16, 2 * 4096 * 4096, device=DEV)
    out = compare({'blocked': lambda: ext.chol_solve_blocked(A, b, mu, sc),
                   'mw': lambda: ext.chol_solve_mw(A, b, mu, sc)},
                  args.warmup, args.runs)
    out['dp_max_abs_diff_over_max_abs'] = rel(
        ext.chol_solve_blocked(A, b, mu, sc)[0],
        ext.chol_solve_mw(A, b, mu, sc)[0])
    out['note'] = 'for information; routing at n <= 4096 is unchanged'
    res['shapes']['16x4096_direct'] = out
    del A, sc

    # the figures behind LIM_4104 of the test, on the test's own inputs
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_chol_blocked import errs, problem  # noqa: E402
    A, b, mu, ref = problem(4104, 2, 61)
    Ad, bd, mud = A.to(DEV), b.to(DEV), mu.to(DEV)
    e_torch = float(errs(torch_blocks(Ad, bd, mud).cpu(), ref).max())
    e_blocked = float(errs(hip_host.chol_solve_damped(Ad, bd, mud).cpu(),
                           ref).max())
    res['n4104_batch2_vs_fp64_host'] = {
        'torch_fp32_blocks': e_torch, 'blocked': e_blocked,
        'limit_4x_torch_capped_5e-2': min(4 * e_torch, 5e-2)}

    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
