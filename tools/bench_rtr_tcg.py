"""Time the RTR inner solve: one ops.rtr_tcg call (k_rtr_tcg, rtr_tcg.hip)
against the torch sequence it replaces (rtr._Objective.grad, rtr._tcg_fixed,
hess_vec) on the same device tensors, eagerly and as captured graphs, and
one rtr.rtr_solve_graphed(maxiter=20) with SAGECAL_RTR_KERNEL on and off.

    python tools/bench_rtr_tcg.py --out profiles/rtr_tcg.json

N = 64 stations (P = 512), maxit = 12, nchunk in {1, 10, 40}, two timeslots
per chunk. kappa = 0 and delta = 1e6 keep every chunk in the loop for all
12 iterations on both paths, so the kernel streams 13 matrices per chunk.
Device events around each call, the paths alternating after warm-up, the
median of 10 with its spread; needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sagecal_amd.ops import dispatch as ops          # noqa: E402
from sagecal_amd.ops import hip_host                 # noqa: E402
from sagecal_amd.ops import reference as R           # noqa: E402
from sagecal_amd.solvers import lm, rtr              # noqa: E402

DEV = 'cuda:0'
N, MAXIT, TPC = 64, 12, 2


def make(nchunk, seed=3):
    """A noisy scalar-coherency problem of nchunk chunks and a start 5 %
    off the truth."""
    rng = np.random.default_rng(seed)
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase, T = len(pairs), TPC * nchunk

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    bb = torch.tensor(np.tile(pairs, (T, 1)))
    rows = (torch.arange(T) // TPC).repeat_interleave(Nbase)
    coh = cplx(T * Nbase)[:, None, None] * torch.eye(2)
    Jt = torch.eye(2) + 0.2 * cplx(nchunk, N, 2, 2)
    x = R.apply_jones(coh, Jt, bb, rows) + 0.01 * cplx(T * Nbase, 2, 2)
    bb, rows = bb.to(DEV), rows.to(DEV)
    c64 = lambda t: t.to(DEV, torch.complex64)
    prob = lm.LMProblem(c64(x), c64(coh), bb, N, nchunk, rows,
                        layout=hip_host.BaselineLayout(bb, Nbase, T, 1, N,
                                                       DEV))
    return prob, c64(Jt + 0.05 * cplx(nchunk, N, 2, 2))


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


def captured(fn):
    """fn as a graph replay, captured after two runs on a side stream."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()                 # the graph's outputs stay allocated
    return lambda: (graph.replay(), keep)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/rtr_tcg.json')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    res = {'tool': 'tools/bench_rtr_tcg.py', 'warmup': args.warmup,
           'runs': args.runs, 'order': 'kernel, torch, kernel, torch, ...',
           'device': 'MI355X (gfx950)', 'N': N, 'P': 8 * N, 'maxit': MAXIT,
           'nchunk': {}}
    for nchunk in (1, 10, 40):
        prob, J = make(nchunk)
        obj = rtr._Objective(prob, rtr._station_iw(prob.bb, N, DEV,
                                                   torch.float32))
        obj.refresh(J)
        delta = torch.full((nchunk,), 1e6, device=DEV)

        def kernel():
            return ops.rtr_tcg(obj.JtJ, obj.Jtr, J, obj.iw, delta, MAXIT, 0.0)

        def torch_seq():
            g = obj.grad(J)
            eta = rtr._tcg_fixed(obj, J, g, delta, MAXIT, 0.0)
            return g, eta, obj.hess_vec(J, eta)
        out = {'eager': compare({'kernel': kernel, 'torch': torch_seq},
                                args.warmup, args.runs),
               'graph': compare({'kernel': captured(kernel),
                                 'torch': captured(torch_seq)},
                                args.warmup, args.runs)}
        *vk, st = kernel()
        vt = torch_seq()
        out['max_abs_diff_over_max_abs'] = {
            k: float((a - b).abs().max() / b.abs().max())
            for k, a, b in zip(('g', 'eta', 'Heta'), vk, vt)}
        out['cg_iterations_entered'] = st[:, 3].tolist()
        nbytes = 13 * 4 * (8 * N) ** 2 * nchunk
        ms = out['graph']['kernel']['ms_median']
        out['bytes_kernel_must_read'] = nbytes
        out['achieved_GB_per_s_graph'] = round(nbytes / ms / 1e6, 1)
        for mode in ('eager', 'graph'):
            out[mode]['torch_over_kernel'] = round(
                out[mode]['torch']['ms_median']
                / out[mode]['kernel']['ms_median'], 2)
        solve = {}
        for name, flag in (('switch_on', '1'), ('switch_off', '0')) * 3:
            os.environ['SAGECAL_RTR_KERNEL'] = flag
            ms, (_, info) = time_ms(
                lambda: rtr.rtr_solve_graphed(prob, J, maxiter=20))
            solve.setdefault(name, []).append(
                {'ms': round(ms, 2),
                 'final_cost': float(info['final_cost'].sum())})
        os.environ.pop('SAGECAL_RTR_KERNEL')
        out['rtr_solve_graphed_maxiter20'] = dict(
            solve, note='three calls each, alternating; the first of each '
            'captures its graph')
        res['nchunk'][str(nchunk)] = out
        print(json.dumps({nchunk: out}), flush=True)

    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
