#!/usr/bin/env python
"""Time one LBFGS cost/gradient evaluation on a GPU, the fused kernels of
lbfgs_mf.hip (SAGECAL_LBFGS_CHANNELS=1) against the per-cluster loop of
hip_host.lbfgs_cost_grad (the switch off), robust cost, at two shapes:

  polish    the -l polish of the default bench.py run: ops.lbfgs_cost_grad
            on bench.build_problem's tile, 64 stations, 960 timeslots
            (1,935,360 rows), 10 clusters, 160 chunks, one channel
            (the channel average), solutions I + 0.1 (randn + i randn).
  bandpass  one minibatch of one mini-band of bench.py --mode bandpass at
            its defaults: stochastic._cost_grad_band_multifreq with the
            consensus terms, 64 stations, 30 of 60 timeslots (60,480 rows),
            10 clusters, one channel of 8 (nsolbw = 8), robust_nu = 10.

Both paths run in one process: 2 warm-up calls of each, then RUNS (default
10) timed calls of each in alternation (fused, loop, fused, loop, ...), a
host clock around the call with torch.cuda.synchronize() on both sides.
Recorded per path: every timing, the median and max - min, the peak of
torch.cuda.max_memory_allocated() above what was allocated before the call,
and the difference between the two paths' results. The fused path counts as
faster where its median is below the loop's by more than the loop's
max - min. Needs a GPU.

    python tools/bench_lbfgs_grad.py --out result.json [--runs N]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                    '..'))
SHAPE = dict(stations=64, dirs=10, srcs=5, tilesz=60, intervals=16, chan=8,
             freq0=150e6, bandwidth=180e3, shapelet_dirs=0, nsolbw=8,
             band_average=False)
WARMUP = 2
SWITCH = 'SAGECAL_LBFGS_CHANNELS'


def polish_shape(bench, torch, dev):
    from sagecal_amd.ops import dispatch as ops
    from sagecal_amd.solvers import sage
    pack, ms, tile, bb = bench.build_problem(SimpleNamespace(**SHAPE), dev,
                                             torch.float32)
    state = sage.CalState(pack, SHAPE['stations'], device=dev,
                          dtype=torch.complex64)
    g = torch.Generator().manual_seed(7)
    J = state.J + 0.1 * torch.view_as_complex(
        torch.randn(*state.J.shape, 2, generator=g)).to(dev)
    cohs = sage.precalc_coherencies(pack, tile).to(torch.complex64)
    x = tile.x.to(torch.complex64)
    T, Nbase = tile.tilesz, tile.Nbase
    info = dict(rows=int(x.shape[0]), channels=1, clusters=pack.M,
                chunks=state.Mt, robust_nu=5.0)
    return info, lambda: ops.lbfgs_cost_grad(
        x, cohs, J, state.chunk_off, state.nchunks, bb, T, Nbase,
        robust_nu=5.0)


def bandpass_shape(bench, torch, dev):
    from sagecal_amd.ops import dispatch as ops
    from sagecal_amd.solvers import stochastic
    args = SimpleNamespace(**dict(SHAPE, intervals=1))
    _, tile, cal = bench.run_bandpass(args, dev, torch.float32, 0, 1)
    bb = tile_bb(tile, cal)          # on the host, as bench.py's
    Nbase = tile.Nbase
    t0, t1 = stochastic.split_minibatches(tile.tilesz, 2)[0]
    rows = slice(t0 * Nbase, t1 * Nbase)
    a, b = cal.bands[0]
    u, v, w = tile.u[rows], tile.v[rows], tile.w[rows]
    fdelta_ch = tile.fdelta / len(tile.freqs)
    cohs_f = [ops.predict_coh(cal.pack, u, v, w, float(tile.freqs[fi]),
                              tile.freq0, fdelta_ch, tile.tdelta,
                              tile.dec0).to(cal.dtype) for fi in range(a, b)]
    stacked = torch.stack(cohs_f)
    xs = tile.xo[a:b, rows].to(cal.dtype).contiguous()
    band = cal.states[0]
    Mt, N = band.J.shape[:2]
    g = torch.Generator().manual_seed(7)
    vv = torch.view_as_real(band.J).reshape(-1) + 0.1 * torch.randn(
        Mt * N * 8, generator=g).to(dev)
    cons = (band.Y, cal._consensus_vec(0), cal.rho_scalar)
    bbm = bb[rows]
    info = dict(rows=int(xs.shape[1]), channels=b - a, clusters=cal.M,
                chunks=Mt, robust_nu=10.0)

    def call():
        # the list for the loop, the stack for the kernels, as
        # _fit_band_multifreq hands them over
        fused = os.environ.get(SWITCH) == '1'
        return stochastic._cost_grad_band_multifreq(
            vv, xs, stacked if fused else cohs_f, cal.chunk_off, cal.nchunks,
            bbm, t1 - t0, Nbase, Mt, N, cal.dtype, 10.0, consensus=cons)
    return info, call


def tile_bb(tile, cal):
    import torch
    N = cal.N
    pairs = [(p, q) for p in range(N) for q in range(p + 1, N)]
    return torch.tensor(pairs * tile.tilesz)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True, help='result JSON path')
    ap.add_argument('--runs', type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_lbfgs_grad: no GPU, nothing to measure')
    import bench
    dev = 'cuda:0'
    paths = (('fused', '1'), ('loop', None))

    def call(fn, switch):
        if switch:
            os.environ[SWITCH] = switch
        try:
            return fn()
        finally:
            os.environ.pop(SWITCH, None)

    res = {'tool': 'tools/bench_lbfgs_grad.py', 'warmup': WARMUP,
           'runs': args.runs, 'order': 'fused, loop, fused, loop, ...',
           'shapes': {}}
    for name, make in (('polish', polish_shape), ('bandpass', bandpass_shape)):
        info, fn = make(bench, torch, dev)
        rec = dict(info, **{p: {'ms_per_call': []} for p, _ in paths})
        outs = {}
        for p, sw in paths:
            for _ in range(WARMUP):
                call(fn, sw)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            outs[p] = call(fn, sw)
            torch.cuda.synchronize()
            rec[p]['peak_bytes_above_inputs'] = \
                torch.cuda.max_memory_allocated() - base
        (cf, gf), (cl, gl) = outs['fused'], outs['loop']
        rec['cost_fused_over_loop_minus_1'] = float(cf) / float(cl) - 1.0
        rec['grad_max_abs_diff_over_max_abs'] = float(
            (gf - gl).abs().max() / gl.abs().max())
        del outs, cf, gf, cl, gl
        for _ in range(args.runs):
            for p, sw in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(fn, sw)
                torch.cuda.synchronize()
                rec[p]['ms_per_call'].append(
                    round((time.perf_counter() - t0) * 1e3, 4))
        for p, _ in paths:
            ms = rec[p]['ms_per_call']
            rec[p]['ms_median'] = round(float(np.median(ms)), 4)
            rec[p]['ms_spread'] = round(max(ms) - min(ms), 4)
        rec['loop_over_fused'] = round(
            rec['loop']['ms_median'] / rec['fused']['ms_median'], 3)
        rec['fused_is_faster'] = bool(
            rec['loop']['ms_median'] - rec['fused']['ms_median']
            > rec['loop']['ms_spread'])
        res['shapes'][name] = rec
        print(f"{name}: fused {rec['fused']['ms_median']:.3f} ms, loop "
              f"{rec['loop']['ms_median']:.3f} ms (spread "
              f"{rec['loop']['ms_spread']:.3f}), peak "
              f"{rec['fused']['peak_bytes_above_inputs'] / 2**20:.1f} / "
              f"{rec['loop']['peak_bytes_above_inputs'] / 2**20:.1f} MiB, "
              f"grad difference {rec['grad_max_abs_diff_over_max_abs']:.2e}",
              flush=True)
        del fn
        torch.cuda.empty_cache()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
