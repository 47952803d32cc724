#!/usr/bin/env python
"""Time beams.predict_coh_withbeam, modes 1-3, on a GPU.

64 stations x 60 timeslots (120,960 rows), 10 clusters x 30 sources, 96
elements per station. 3 warm-up calls, then 20 calls timed one by one with
device events; the events bracket the whole call, host-side beam work
included. Needs a GPU. Uses only interfaces that predate the beam kernels,
so `--tree` can point it at another checkout of this repository (built in
place) to compare revisions: run the trees in alternation from one job,
each in its own process. A mode that raises is recorded with its exception
text instead of timings. `--cpu-mode2 CALLS` adds wall-clock timings of
mode 2 on CPU tensors at the same size, the baseline where a revision has
no working GPU path for it.

`--two-stage` makes every station a two-stage HBA beamformer: `--elements`
tile centroids and 16 dipoles per tile, tile pointing 0.02 rad off the
station pointing; it needs a tree that has the two-stage model. The
work-equivalent single-stage call, on any tree, is `--elements` = tiles + 16
(the same number of phasors per station). `--gain-channels F` also times
the station gains of F channels: F single-frequency array_beam_gains calls
and, where the tree has it, one batched station_beam_gains call.
`--element-channels F` times the dipole element E-Jones of F channels from
the `--elem-type` table over the tool's timeslots x sources directions: the
per-channel host loop (numpy pattern, cast to complex64, copy to the device;
1 warm-up pass and 3 timed ones, each takes seconds) against one batched
beams.element_jones_channels call on the device, upload of the directions
included.

    python tools/bench_beam_predict.py --out result.json [--tree DIR]
        [--cpu-mode2 CALLS] [--sample sample.pt] [--modes 1,2,3]
        [--elements E] [--two-stage] [--gain-channels F]
        [--element-channels F --elem-type {lba,hba,alo}]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

STATIONS, TSLOTS, DIRS, SRCS, ELEMS = 64, 60, 10, 30, 96
FREQ0, FDELTA, TDELTA, DEC0 = 150e6, 60e3, 10.0, np.pi / 4
LON, LAT, TMJD0 = 0.1, 0.92, 57000.0
WARMUP, CALLS = 3, 20


TILE_DIPOLES, TILE_OFFSET = 16, (0.02, -0.014)


def make_inputs(torch, elements=ELEMS, two_stage=False):
    from sagecal_amd import beams, msdata, sky
    from sagecal_amd.ops.reference import SourcePack
    srcs, clist = sky.make_synthetic_sky(M=DIRS, nsrc_per_cluster=SRCS,
                                         seed=17)
    pack = SourcePack(sky.build_clusters(srcs, clist, 0.0, DEC0, FREQ0))
    ms = msdata.SyntheticMS(N=STATIONS, tilesz=TSLOTS, Ntime=TSLOTS, Nchan=1,
                            pack=None, seed=13, tdelta=TDELTA)
    tile = ms.load_tile(0)
    rng = np.random.default_rng(29)
    elems = [rng.uniform(-30, 30, (elements, 3)) for _ in range(STATIONS)]
    kw = {}
    if two_stage:
        kw = dict(bf_type='tile', tile_ra0=TILE_OFFSET[0],
                  tile_dec0=DEC0 + TILE_OFFSET[1],
                  tile_enu=rng.uniform(-2.5, 2.5,
                                       (STATIONS, TILE_DIPOLES, 3)))
    cfg = beams.ArrayConfig(elems, LON, LAT, 0.0, DEC0, **kw)
    tmjd = TMJD0 + (np.arange(TSLOTS) + 0.5) * TDELTA / 86400.0
    return pack, (tile.u, tile.v, tile.w), ms.bb_tensor(device='cpu'), \
        ms.Nbase, cfg, tmjd


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True, help='result JSON path')
    ap.add_argument('--tree', default=None,
                    help='repository checkout to import sagecal_amd from')
    ap.add_argument('--cpu-mode2', type=int, default=0, metavar='CALLS',
                    help='also time mode 2 on the CPU this many times')
    ap.add_argument('--sample', default=None,
                    help='save every 997th output row of each mode here')
    ap.add_argument('--label', default='')
    ap.add_argument('--modes', default='1,2,3',
                    help='comma-separated predict modes to time')
    ap.add_argument('--elements', type=int, default=ELEMS,
                    help='elements (tile centroids with --two-stage) per '
                         'station')
    ap.add_argument('--two-stage', action='store_true',
                    help='two-stage HBA stations: 16 dipoles per tile')
    ap.add_argument('--gain-channels', type=int, default=0, metavar='F',
                    help='also time the station gains of F channels')
    ap.add_argument('--element-channels', type=int, default=0, metavar='F',
                    help='also time the element E-Jones of F channels')
    ap.add_argument('--elem-type', default='hba',
                    choices=['lba', 'hba', 'alo'],
                    help='coefficient table of --element-channels')
    args = ap.parse_args()
    tree = os.path.abspath(args.tree or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), '..'))
    sys.path.insert(0, tree)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_beam_predict: no GPU, nothing to measure')
    from sagecal_amd import beams
    dev = torch.device('cuda:0')
    pack, uvw, bb, Nbase, cfg, tmjd = make_inputs(torch, args.elements,
                                                  args.two_stage)
    uvw_d = [t.to(dev) for t in uvw]
    bb_d = bb.to(dev)
    res = {'label': args.label, 'tree': os.path.basename(tree),
           'rows': int(uvw[0].shape[0]), 'stations': STATIONS,
           'timeslots': TSLOTS, 'clusters': DIRS, 'sources': DIRS * SRCS,
           'elements': args.elements, 'two_stage': args.two_stage,
           'dipoles_per_tile': TILE_DIPOLES if args.two_stage else 0,
           'warmup': WARMUP, 'calls': CALLS, 'modes': {}}
    samples = {}
    tag = args.label or res['tree']

    def predict(mode, rows, pairs):
        return beams.predict_coh_withbeam(
            pack, *rows, FREQ0, FREQ0, FDELTA, TDELTA, DEC0, cfg, tmjd,
            pairs, Nbase, TSLOTS, mode=mode)

    def timed(fn, warmup=WARMUP, calls=CALLS):
        """Median-ready list of `calls` device-event timings of fn(), ms."""
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, out

    def stats(ms):
        return {'ms_per_call': [round(x, 4) for x in ms],
                'ms_median': round(float(np.median(ms)), 4),
                'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}

    if args.gain_channels > 0:
        # channel gains alone, geometry prebuilt: F single-frequency calls
        # against one batched call; any exception ends the job
        F = args.gain_channels
        freqs = [FREQ0 + (i - (F - 1) / 2) * FDELTA / F for i in range(F)]
        geom = beams.beam_geometry(cfg, *beams._pack_radec(pack, DEC0), tmjd)
        res['gains'] = {'channels': F, 'freqs': freqs}
        ms, rows = timed(lambda: [beams.array_beam_gains(cfg, geom, f, dev)
                                  for f in freqs])
        res['gains']['per_channel_calls'] = stats(ms)
        print(f'{tag} gains, {F} single-frequency calls: median '
              f'{np.median(ms):.3f} ms', flush=True)
        if hasattr(beams, 'station_beam_gains'):
            ms, batch = timed(lambda: beams.station_beam_gains(
                cfg, geom, freqs, dev))
            res['gains']['batched_call'] = stats(ms)
            res['gains']['batched_vs_per_channel_max_abs'] = float(
                (batch - torch.stack(rows)).abs().max())
            print(f'{tag} gains, one batched call: median '
                  f'{np.median(ms):.3f} ms', flush=True)
            samples['gains'] = batch[:, ::7, ::13].cpu()
        else:
            samples['gains'] = torch.stack(rows)[:, ::7, ::13].cpu()

    if args.element_channels > 0:
        # element E-Jones alone, geometry prebuilt: the per-channel host
        # evaluation against one batched device call; any exception ends
        # the job
        F = args.element_channels
        co = beams.LofarElementCoeffs.load(args.elem_type)
        fr = co.freqs_ghz * 1e9
        freqs = np.linspace(fr[0], fr[-1], F + 2)[1:-1].tolist()
        geom = beams.beam_geometry(cfg, *beams._pack_radec(pack, DEC0), tmjd)
        res['element'] = {'channels': F, 'elem_type': args.elem_type,
                          'freqs': freqs, 'directions': geom.T * geom.K}
        ms, rows = timed(lambda: [
            beams.element_jones(co, geom, f).to(torch.complex64).to(dev)
            for f in freqs], warmup=1, calls=3)
        res['element']['host_loop'] = dict(stats(ms), warmup=1, calls=3)
        print(f'{tag} element E-Jones, {F} host evaluations + copies: '
              f'median {np.median(ms):.1f} ms', flush=True)
        ms, batch = timed(lambda: beams.element_jones_channels(
            co, geom, freqs, dev))
        res['element']['device_call'] = stats(ms)
        rows = torch.stack(rows)
        res['element']['device_vs_host_max_rel'] = float(
            (batch - rows).abs().max() / rows.abs().max())
        print(f'{tag} element E-Jones, one batched device call: median '
              f'{np.median(ms):.3f} ms', flush=True)
        samples['element'] = batch[:, ::7, ::13].cpu()

    for mode in [int(m) for m in args.modes.split(',') if m]:
        try:
            for _ in range(WARMUP):
                out = predict(mode, uvw_d, bb_d)
            torch.cuda.synchronize()
        except Exception as e:          # recorded as this tree's result
            text = f'{type(e).__name__}: {e}'.strip()
            res['modes'][str(mode)] = {'error': text[:600]}
            print(f'{tag} mode {mode}: raised {text[:200]}', flush=True)
            if 'HIP' in text or 'illegal' in text:
                break                   # device error: start nothing more
            continue
        ms = []
        for _ in range(CALLS):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = predict(mode, uvw_d, bb_d)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res['modes'][str(mode)] = {
            'ms_per_call': [round(x, 4) for x in ms],
            'ms_median': round(float(np.median(ms)), 4),
            'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}
        samples[str(mode)] = out[:, ::997].cpu()
        print(f'{tag} mode {mode}: median {np.median(ms):.3f} ms  '
              f'min {min(ms):.3f}  max {max(ms):.3f}', flush=True)
        del out
    if args.cpu_mode2 > 0:
        ms = []
        for _ in range(args.cpu_mode2):
            t0 = time.perf_counter()
            predict(2, uvw, bb)
            ms.append((time.perf_counter() - t0) * 1e3)
            print(f'{tag} mode 2 on the CPU: {ms[-1]:.1f} ms', flush=True)
        res['cpu_mode2'] = {
            'what': 'mode 2 on CPU tensors, wall clock, per-source loop',
            'threads': torch.get_num_threads(), 'calls': len(ms),
            'ms_per_call': [round(x, 2) for x in ms],
            'ms_median': round(float(np.median(ms)), 2)}
    if args.sample:
        torch.save(samples, args.sample)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
