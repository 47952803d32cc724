#!/usr/bin/env python
"""Time hip_host.predict_coh on skies with shapelet sources.

Row count of the SKA-scale configuration (512 stations x 10 timeslots =
1,308,160 rows), 50 clusters x 4 sources, two skies:
  few : 2 shapelet sources with n0=3 (what `bench.py --shapelet-dirs 2`
        makes)
  many: 32 shapelet sources with n0=8
3 warm-up calls, then 20 calls timed one by one with device events. Needs
a GPU; there is no CPU fallback. Uses only interfaces that predate the
shapelet kernel, so `--tree` can point it at another checkout of this
repository (built in place) to compare revisions: run the trees in
alternation from one job, each in its own process.

    python tools/bench_shapelet_predict.py --out result.json [--tree DIR]
        [--host-mirror] [--sample sample.pt]
"""
import argparse
import json
import os
import sys

import numpy as np

STATIONS, TSLOTS, DIRS, SRCS = 512, 10, 50, 4
FREQ0, FDELTA, TDELTA, DEC0 = 150e6, 60e3, 10.0, np.pi / 4
SKIES = {'few': (2, 3), 'many': (32, 8)}      # name: (shapelets, n0)
WARMUP, CALLS = 3, 20


def make_pack(nshap, n0):
    from sagecal_amd import sky
    from sagecal_amd.ops.reference import SourcePack
    srcs, clist = sky.make_synthetic_sky(M=DIRS, nsrc_per_cluster=SRCS,
                                         seed=17)
    rng = np.random.default_rng(23)
    k = np.arange(n0)
    decay = 1.0 / (1.0 + k[None, :] + k[:, None]) ** 2
    for ci in range(nshap):
        s = srcs[clist[ci][2][0]]
        s.stype = 4
        s.eX = s.eY = 1.0
        s.sh_n0 = n0
        s.sh_beta = 1e-3
        s.sh_coeff = (rng.standard_normal((n0, n0)) * decay).reshape(-1)
    return SourcePack(sky.build_clusters(srcs, clist, 0.0, DEC0, FREQ0))


def make_uvw(torch, dev):
    """Seeded uvw in seconds with the spread of a ~20 km array."""
    g = torch.Generator().manual_seed(31)
    R = STATIONS * (STATIONS - 1) // 2 * TSLOTS
    uvw = (torch.rand(3, R, generator=g, dtype=torch.float64) - 0.5) * 1.4e-4
    uvw[2] *= 0.1
    return [t.contiguous().to(dev) for t in uvw]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True, help='result JSON path')
    ap.add_argument('--tree', default=None,
                    help='repository checkout to import sagecal_amd from')
    ap.add_argument('--host-mirror', action='store_true',
                    help='time the torch mirror (SAGECAL_SHAPELET_HOST=1)')
    ap.add_argument('--sample', default=None,
                    help='save every 997th output row of each sky here')
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    tree = os.path.abspath(args.tree or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), '..'))
    sys.path.insert(0, tree)
    if args.host_mirror:
        os.environ['SAGECAL_SHAPELET_HOST'] = '1'
    else:
        os.environ.pop('SAGECAL_SHAPELET_HOST', None)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_shapelet_predict: no GPU, nothing to measure')
    from sagecal_amd.ops import hip_host
    dev = torch.device('cuda:0')
    u, v, w = make_uvw(torch, dev)
    res = {'label': args.label, 'tree': os.path.basename(tree),
           'host_mirror': bool(args.host_mirror), 'rows': int(u.shape[0]),
           'clusters': DIRS, 'sources': DIRS * SRCS, 'warmup': WARMUP,
           'calls': CALLS, 'skies': {}}
    samples = {}
    for name, (nshap, n0) in SKIES.items():
        pack = make_pack(nshap, n0)
        call = lambda: hip_host.predict_coh(pack, u, v, w, FREQ0, FREQ0,
                                            FDELTA, TDELTA, DEC0)
        for _ in range(WARMUP):
            out = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(CALLS):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res['skies'][name] = {
            'shapelet_sources': nshap, 'n0': n0,
            'ms_per_call': [round(x, 4) for x in ms],
            'ms_median': round(float(np.median(ms)), 4),
            'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}
        samples[name] = out[:, ::997].cpu()
        print(f"{args.label or res['tree']} {name}: median "
              f"{np.median(ms):.3f} ms  min {min(ms):.3f}  max {max(ms):.3f}",
              flush=True)
        del out, pack
    if args.sample:
        torch.save(samples, args.sample)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
