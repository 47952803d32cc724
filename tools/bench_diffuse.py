"""Time the diffuse-cluster predict with the spatial model: ops.diffuse_
coherencies through k_diffuse_station and k_diffuse_pair (diffuse.hip)
against the host path it replaces (u, v, w to the host,
shapelet.recalculate_diffuse_coherencies in complex128, the result cast to
complex64 and copied back), on the same inputs.

    python tools/bench_diffuse.py --out profiles/diffuse.json

Section `bench`: 64 stations, T = 60, Gz = 3, Gc = 10 (n2 = 14, 2016 pairs,
120,960 rows). Kernels: device events, the median of 10 after 2 warm-ups,
with the 3 host calls in between the first three; the host calls are all
reported. Peak device memory above the inputs, and the error of the kernels
against the host result. Section `cases`: the error of the kernels at the
shapes tests/test_gpu_diffuse.py checks. Each section runs in a process of
its own under its own time limit, and a section that fails ends the run;
needs a GPU."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sagecal_amd import shapelet                     # noqa: E402
from sagecal_amd.ops import dispatch as ops          # noqa: E402

DEV = 'cuda:0'
FREQ, FDELTA, BETA_Z, BETA_C = 150e6, 1e6, 0.02, 0.01
LMN = (0.01, -0.02, math.sqrt(1 - 0.01 ** 2 - 0.02 ** 2) - 1)
LIMITS = {'bench': 420, 'cases': 180}       # seconds per section
CASES = [(3, 1, 1, 1), (5, 2, 3, 3), (6, 3, 6, 2), (4, 3, 13, 2),
         (4, 4, 26, 1)]


def make(N, Gz, Gc, T, seed=11):
    """Seeded float64 draws on the device with |u f g2|, |v f g2| < 3, all
    pairs p < q: the timings depend on the shapes alone."""
    rng = np.random.default_rng(seed)
    cplx = lambda *s: torch.tensor(rng.standard_normal(s)
                                   + 1j * rng.standard_normal(s))
    g2 = shapelet.product_scale(
        BETA_Z, shapelet.product_scale(BETA_C, BETA_Z))
    pairs = torch.tensor([(p, q) for p in range(N) for q in range(p + 1, N)],
                         dtype=torch.int32, device=DEV)
    u, v, w = (torch.tensor(rng.uniform(-3, 3, T * len(pairs)), device=DEV)
               / (FREQ * g2) for _ in range(3))
    return u, v, w, pairs, cplx(N, Gz * Gz, 2, 2), cplx(Gc * Gc, 2, 2)


def kernels(u, v, w, pairs, Z, Cm, T):
    return ops.diffuse_coherencies(u, v, w, pairs, T, Z, BETA_Z, Cm, BETA_C,
                                   LMN, FREQ, FDELTA)


def host(u, v, w, pairs, Z, Cm, T):
    """What ConsensusADMM.diffuse_coherencies and the hook do without the
    kernels."""
    out = shapelet.recalculate_diffuse_coherencies(
        u.cpu().double(), v.cpu().double(), w.cpu().double(),
        pairs.cpu().long().repeat(T, 1), Z, BETA_Z, Cm, BETA_C, *LMN, FREQ,
        FDELTA)
    return out.to(device=u.device, dtype=torch.complex64)


def rel_err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def section_bench(args):
    N, Gz, Gc, T = 64, 3, 10, 60
    inp = make(N, Gz, Gc, T)
    for _ in range(args.warmup):
        kernels(*inp, T)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = kernels(*inp, T)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms, host_s, ref = [], [], None
    for i in range(args.runs):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        kernels(*inp, T)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        if i < args.host_runs:
            t0 = time.perf_counter()
            ref = host(*inp, T)
            torch.cuda.synchronize()
            host_s.append(time.perf_counter() - t0)
    med = statistics.median(ms)
    return {'N': N, 'Gz': Gz, 'Gc': Gc, 'T': T, 'n2': Gc + 2 * Gz - 2,
            'pairs': int(inp[3].shape[0]), 'rows': int(inp[0].shape[0]),
            'kernels': {'ms_per_call': [round(x, 4) for x in ms],
                        'ms_median': round(med, 4),
                        'ms_spread': round(max(ms) - min(ms), 4),
                        'peak_bytes_above_inputs': peak,
                        'output_bytes': out.numel() * 8},
            'host_path': {'s_per_call': [round(x, 3) for x in host_s],
                          's_median': round(statistics.median(host_s), 3)},
            'speedup_of_medians': round(
                1e3 * statistics.median(host_s) / med, 1),
            'rel_err_kernels_to_host_complex64': rel_err(out, ref)}


def section_cases(args):
    res = []
    for N, Gz, Gc, T in CASES:
        inp = make(N, Gz, Gc, T)
        ref = shapelet.recalculate_diffuse_coherencies(
            *(t.cpu() for t in inp[:3]), inp[3].cpu().long().repeat(T, 1),
            inp[4], BETA_Z, inp[5], BETA_C, *LMN, FREQ, FDELTA)
        res.append({'N': N, 'Gz': Gz, 'Gc': Gc, 'T': T,
                    'n2': Gc + 2 * Gz - 2,
                    'rel_err': rel_err(kernels(*inp, T).cpu(), ref)})
    return {'limit': 1e-5, 'reference': 'host path in complex128',
            'error': 'max |V - ref| / max |ref|', 'cases': res}


SECTIONS = {'bench': section_bench, 'cases': section_cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/diffuse.json')
    ap.add_argument('--sections', default='bench,cases')
    ap.add_argument('--section', help='run this one section and print it')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--host-runs', type=int, default=3)
    args = ap.parse_args()
    if args.section:
        assert torch.cuda.is_available(), 'needs a GPU'
        print(json.dumps(SECTIONS[args.section](args)), flush=True)
        return
    res = {'tool': 'tools/bench_diffuse.py', 'warmup': args.warmup,
           'runs': args.runs, 'host_runs': args.host_runs,
           'order': 'a kernel call, then a host call while there are any',
           'device': 'MI355X (gfx950)'}
    for name in args.sections.split(','):
        # a fresh process per section, ended at its limit; a section that
        # fails or hangs ends the run
        done = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--section', name,
             '--warmup', str(args.warmup), '--runs', str(args.runs),
             '--host-runs', str(args.host_runs)],
            stdout=subprocess.PIPE, text=True, timeout=LIMITS[name],
            check=True)
        res[name] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps({name: res[name]}), flush=True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
