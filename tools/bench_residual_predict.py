#!/usr/bin/env python
"""Time sage.calculate_residuals_multifreq and sage.precalc_coherencies on a
GPU, the all-channels kernels against the per-channel loop
(SAGECAL_RESIDUAL_LOOP=1), at the shape of the default bench.py run: 64
stations, tilesz 60 x 16 intervals (1,935,360 rows), 8 channels, 10
clusters of 5 sources, 16 solution chunks per cluster. The problem is
bench.build_problem's; the solutions are I + 0.1 (randn + i randn).

Both paths run in one process, in alternation: 2 warm-up calls of each,
then RUNS (default 10) timed calls of each, a host clock around the call
with torch.cuda.synchronize() on both sides. Recorded per path: every
timing and the median, the peak of torch.cuda.max_memory_allocated()
above what was allocated before the call, and the largest difference
between the two paths' outputs. Needs a GPU.

    python tools/bench_residual_predict.py --out result.json [--runs N]

--beam MODE (1: station gains, 2: gains and element patterns, 3: patterns
alone; the -B 1/4, 2/5 and 3/6 of the command line) times the beamed paths
on the same workload instead: random gains [F, T, K, N] in [0.2, 1] and
random patterns [F, T, K, 2, 2] (one per source, NE = 1), given to
calculate_residuals_multifreq as beam= together with the coh_fn of the
per-channel loop, and the wideband solve model of -B 4/5/6, the channel
mean of the beamed predicts: one predict_coh_channels(reduce='mean') call
against the loop over predict_coh. The loop is what runs without the
all-channels kernels, selected by the same switch.

Kernel durations come from a second run under the profiler, which slows
the host and so gets no timings of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \\
        python tools/bench_residual_predict.py --profile-run
    python tools/bench_residual_predict.py --out result.json \\
        --merge-kernels DIR/.../NAME_kernel_stats.csv

--profile-run calls each path PROFILE_CALLS times and writes nothing;
--merge-kernels adds the rows of the kernels named k_* to an existing
result file and needs no GPU.
"""
import argparse
import csv
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                    '..'))
SHAPE = dict(stations=64, dirs=10, srcs=5, tilesz=60, intervals=16, chan=8,
             freq0=150e6, bandwidth=180e3, shapelet_dirs=0)
WARMUP, PROFILE_CALLS = 2, 2
SWITCH = 'SAGECAL_RESIDUAL_LOOP'


def merge_kernels(out, stats_csv):
    with open(out) as f:
        res = json.load(f)
    rows = []
    with open(stats_csv, newline='') as f:
        for r in csv.DictReader(f):
            if r['Name'].startswith('k_'):
                rows.append({'name': r['Name'], 'calls': int(r['Calls']),
                             'total_ms': round(int(r['TotalDurationNs'])
                                               / 1e6, 4),
                             'average_us': round(float(r['AverageNs'])
                                                 / 1e3, 2)})
    res['kernel_trace'] = {
        'what': f'--profile-run under rocprofv3 --kernel-trace --stats: '
                f'{PROFILE_CALLS} calls of each function on each path',
        'kernels': rows}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)


def beamed_functions(mode, sage, state, pack, tile, bb):
    """The two timed functions with the beam of `mode`, each taking the
    all-channels kernel or the per-channel loop by the switch."""
    import torch
    from sagecal_amd.ops import dispatch as ops
    from sagecal_amd.ops import hip_host
    dev = tile.u.device
    F, N, Nbase = len(tile.freqs), SHAPE['stations'], tile.Nbase
    T, K = tile.tilesz, int(pack.cluster_off[-1])
    g = torch.Generator().manual_seed(11)
    bm = {}
    if mode in (1, 2):
        bm['beam'] = (0.2 + 0.8 * torch.rand(F, T, K, N, generator=g)).to(dev)
    if mode in (2, 3):
        bm['ejones'] = torch.view_as_complex(
            2.0 * torch.rand(F, T, K, 2, 2, 2, generator=g) - 1.0).to(dev)
    pairs = bb[:Nbase].to(torch.int32).contiguous()
    freqs = [float(f) for f in tile.freqs]
    fdch = tile.fdelta / F

    def coh_fn(f):
        fi = freqs.index(f)
        return hip_host.predict_coh(
            pack, tile.u, tile.v, tile.w, f, tile.freq0, fdch, tile.tdelta,
            tile.dec0, pairs=pairs, Nbase=Nbase,
            beam=bm['beam'][fi] if 'beam' in bm else None,
            ejones=bm['ejones'][fi].unsqueeze(2) if 'ejones' in bm else None)

    def mean_predict():
        if sage._all_channels_ok(pack, tile.u):
            return ops.predict_coh_channels(
                pack, tile.u, tile.v, tile.w, freqs, tile.freq0, fdch,
                tile.tdelta, tile.dec0, reduce='mean', pairs=pairs,
                Nbase=Nbase, **bm)
        acc = None
        for f in freqs:
            c = coh_fn(f)
            acc = c if acc is None else acc + c
        return acc / F

    return {'calculate_residuals_multifreq':
            lambda: sage.calculate_residuals_multifreq(
                state, pack, tile, bb, coh_fn=coh_fn, beam=bm),
            'wideband_mean_predict': mean_predict}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='result JSON path')
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--beam', type=int, choices=(1, 2, 3), metavar='MODE')
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--merge-kernels', metavar='CSV')
    args = ap.parse_args()
    if args.merge_kernels:
        merge_kernels(args.out, args.merge_kernels)
        return
    if not args.profile_run and not args.out:
        ap.error('--out is required')
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_residual_predict: no GPU, nothing to measure')
    import bench
    from sagecal_amd.solvers import sage
    dev = 'cuda:0'
    pack, ms, tile, bb = bench.build_problem(SimpleNamespace(**SHAPE), dev,
                                             torch.float32)
    state = sage.CalState(pack, SHAPE['stations'], device=dev,
                          dtype=torch.complex64)
    g = torch.Generator().manual_seed(7)
    state.J = state.J + 0.1 * torch.view_as_complex(
        torch.randn(*state.J.shape, 2, generator=g)).to(dev)

    def call(fn, loop):
        if loop:
            os.environ[SWITCH] = '1'
        try:
            return fn()
        finally:
            os.environ.pop(SWITCH, None)

    fns = {'calculate_residuals_multifreq':
           lambda: sage.calculate_residuals_multifreq(state, pack, tile, bb),
           'precalc_coherencies':
           lambda: sage.precalc_coherencies(pack, tile)}
    if args.beam:
        fns = beamed_functions(args.beam, sage, state, pack, tile, bb)
    paths = (('fused', False), ('loop', True))

    if args.profile_run:
        for fn in fns.values():
            for _name, loop in paths:
                for _ in range(PROFILE_CALLS):
                    call(fn, loop)
        torch.cuda.synchronize()
        return

    res = {'tool': 'tools/bench_residual_predict.py',
           'rows': int(tile.u.shape[0]), 'channels': len(tile.freqs),
           'clusters': pack.M, 'sources': int(pack.cluster_off[-1]),
           'chunks': state.Mt, 'warmup': WARMUP, 'runs': args.runs,
           'beam_mode': args.beam,
           'order': 'fused, loop, fused, loop, ...', 'functions': {}}
    for name, fn in fns.items():
        rec = {p: {'ms_per_call': []} for p, _ in paths}
        outs = {}
        for p, loop in paths:
            for _ in range(WARMUP):
                call(fn, loop)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            outs[p] = call(fn, loop)
            torch.cuda.synchronize()
            rec[p]['peak_bytes_above_start'] = \
                torch.cuda.max_memory_allocated() - base
            rec[p]['output_bytes'] = outs[p].numel() * outs[p].element_size()
        # residuals: against the largest subtracted visibility; coherencies:
        # against the largest coherency
        scale = (tile.xo - outs['loop']).abs().max() \
            if name.startswith('calculate') else outs['loop'].abs().max()
        rec['fused_vs_loop_max_abs_over_scale'] = float(
            (outs['fused'] - outs['loop']).abs().max() / scale)
        del outs
        for _ in range(args.runs):
            for p, loop in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(fn, loop)
                torch.cuda.synchronize()
                rec[p]['ms_per_call'].append(
                    round((time.perf_counter() - t0) * 1e3, 4))
        for p, _ in paths:
            rec[p]['ms_median'] = round(
                float(np.median(rec[p]['ms_per_call'])), 4)
        rec['loop_over_fused'] = round(
            rec['loop']['ms_median'] / rec['fused']['ms_median'], 3)
        res['functions'][name] = rec
        print(f"{name}: fused {rec['fused']['ms_median']:.3f} ms, loop "
              f"{rec['loop']['ms_median']:.3f} ms, peak "
              f"{rec['fused']['peak_bytes_above_start'] / 2**20:.0f} / "
              f"{rec['loop']['peak_bytes_above_start'] / 2**20:.0f} MiB, "
              f"difference {rec['fused_vs_loop_max_abs_over_scale']:.2e}",
              flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
