"""Time the influence-map leverage: diagnostics.leverage through k_leverage
(leverage.hip) against its torch paths on the same device tensors, and
diagnostics.influence_map(cluster=None) at the default bench.py shape, split
into JtJ assembly, float64 inverse and k_leverage.

    python tools/bench_leverage.py --out profiles/leverage.json

Shape (a): 64 stations, one cluster, 8 timeslots, one chunk (16,128 rows):
the kernel path (T and Nbase given), the torch path of ops.leverage_rows
(SAGECAL_FORCE_REFERENCE=1, blocks per chunk and pair) and the per-row gather
that diagnostics.leverage does without T and Nbase (about 34 GB). Shape (b):
64 stations, 960 timeslots, 10 clusters of 16 chunks (1,935,360 rows), kernel
only. Device events around each call, the paths alternating after warm-up,
the median of 10 with its spread and the peak memory; needs a GPU.

    python tools/bench_leverage.py --sections b_bench_default,c_ten_chunks \
        --out profiles/spd_inverse.json

also times the float64 inverse kernels of spd_inverse.hip
(ops.spd_inverse_damped) next to torch.linalg.inv in shape (b), 160 matrices
of 512 from the float32 JtJ, and in shape (c), the 10 matrices of one chunk
per cluster; at mu = 1e-6 as the diagnostic sets it and at 1e-2, with the
number of matrices the kernels flag as not positive definite (their last
kernel skips those, and the diagnostic sends them to torch.linalg.inv), and
influence_map(cluster=None) with SAGECAL_INVERSE_KERNEL=1 and without.

    python tools/bench_leverage.py --sections d_normal_f64 \
        --out profiles/normal_f64.json

times the float64 assembly of normal_f64.hip (ops.normal_matrices) in shape
(b) against the ten float32 ops.jtj_jtr calls it replaces, counts the
matrices the inverse kernels flag for either, and times the whole map with
SAGECAL_NORMAL_F64=1 and SAGECAL_INVERSE_KERNEL=1, the latter alone, and
neither."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sagecal_amd.ops import dispatch as ops          # noqa: E402
from sagecal_amd.ops import hip_host                 # noqa: E402
from sagecal_amd.ops import reference as R           # noqa: E402
from sagecal_amd.solvers import diagnostics as diag  # noqa: E402
from sagecal_amd.solvers import sage                 # noqa: E402

DEV = 'cuda:0'
N = 64


def make(T, nchunks, seed=3):
    """Seeded noise data, coherencies and J = I + 0.2 noise on the device:
    the timings depend on the shapes alone."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cplx = lambda *s: torch.view_as_complex(
        torch.randn(*s, 2, device=DEV, generator=g))
    pairs = [(p, q) for p in range(N) for q in range(p + 1, N)]
    Nbase, M = len(pairs), len(nchunks)
    bb = torch.tensor(pairs, device=DEV).repeat(T, 1)
    state = sage.CalState(types.SimpleNamespace(M=M, nchunk=nchunks), N,
                          device=DEV, dtype=torch.complex64)
    state.J = state.J + 0.2 * cplx(*state.J.shape)
    tile = types.SimpleNamespace(tilesz=T, Nbase=Nbase,
                                 x=cplx(T * Nbase, 2, 2))
    return state, cplx(M, T * Nbase, 2, 2), tile, bb


def time_ms(fn):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def compare(fns, warmup, runs):
    """Alternate the callables of `fns` {name: fn}; per name the timings
    and the peak memory of one call."""
    peak = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(time_ms(fn)[0])
    return {k: {'ms_per_call': [round(x, 4) for x in v],
                'ms_median': round(statistics.median(v), 4),
                'ms_spread': round(max(v) - min(v), 4),
                'peak_bytes_above_inputs': peak[k]} for k, v in ms.items()}


def forced_reference(fn):
    def run():
        os.environ['SAGECAL_FORCE_REFERENCE'] = '1'
        try:
            return fn()
        finally:
            os.environ.pop('SAGECAL_FORCE_REFERENCE')
    return run


def with_inverse_kernel(fn):
    def run():
        os.environ['SAGECAL_INVERSE_KERNEL'] = '1'
        try:
            return fn()
        finally:
            os.environ.pop('SAGECAL_INVERSE_KERNEL')
    return run


def inverse_paths(JtJ):
    """The callables that invert JtJ + mu I, and what the kernels flag."""
    fns = {'inverse_float64': lambda: diag._damped_inverse(JtJ, 1e-6),
           'inverse_kernels': lambda: ops.spd_inverse_damped(JtJ, 1e-6),
           'inverse_float64_mu1e-2': lambda: ops.spd_inverse_torch(JtJ, 1e-2),
           'inverse_kernels_mu1e-2': lambda: ops.spd_inverse_damped(JtJ,
                                                                    1e-2)}
    flagged = {f'mu{mu:g}': int(hip_host.spd_inverse_damped(
        JtJ, mu, return_info=True)[1].count_nonzero()) for mu in (1e-6, 1e-2)}
    ref, X = fns['inverse_float64_mu1e-2'](), fns['inverse_kernels_mu1e-2']()
    return fns, {'matrices': int(JtJ.shape[0]), 'n': int(JtJ.shape[1]),
                 'kernels_flag_not_positive_definite': flagged,
                 'max_abs_diff_mu1e-2': float((X - ref).abs().max()),
                 'max_abs_inverse_mu1e-2': float(ref.abs().max())}


def shape_a(args):
    T = 8
    state, cohs, tile, bb = make(T, [1])
    lay = hip_host.BaselineLayout(bb, tile.Nbase, T, 1, N, DEV)
    call = lambda **kw: diag.leverage(tile.x, cohs[0], state.J, bb, N,
                                      layout=lay, **kw)
    fns = {'kernel': lambda: call(T=T, Nbase=tile.Nbase),
           'torch_per_chunk_and_pair': forced_reference(
               lambda: call(T=T, Nbase=tile.Nbase)),
           'torch_per_row_gather': forced_reference(call)}
    out = compare(fns, args.warmup, args.runs)
    ref = fns['torch_per_row_gather']()
    out['max_abs_diff_to_per_row_gather'] = {
        k: float((fns[k]() - ref).abs().max()) for k in list(fns)[:2]}
    out['rows'] = T * tile.Nbase
    return out


def shape_b(args):
    T, M, K = 960, 10, 16
    state, cohs, tile, bb = make(T, [K] * M)
    Nbase, Rn = tile.Nbase, T * tile.Nbase
    lay = hip_host.BaselineLayout(bb, Nbase, T, 1, N, DEV)
    rows = R.chunk_rows_for(0, state.nchunks, T, Nbase, Rn, DEV)
    tab = ops.lbfgs_chunk_table(state.chunk_off, state.nchunks, T, DEV)
    pairs = ops.lbfgs_pair_table(bb, Nbase, DEV)

    def assemble():
        return torch.cat([
            ops.jtj_jtr(tile.x, cohs[ci], state.cluster_J(ci), bb, N, None,
                        rows, K, lay)[0] for ci in range(M)])
    JtJ = assemble()
    Hinv = diag._damped_inverse(JtJ, 1e-6)
    inv_fns, inv_facts = inverse_paths(JtJ)
    imap = lambda: diag.influence_map(state, cohs, tile, bb, cluster=None,
                                      layout=lay)
    out = compare({
        'jtj_assembly': assemble, **inv_fns,
        'k_leverage': lambda: ops.leverage_rows(cohs, state.J, Hinv, tab,
                                                pairs),
        'influence_map_all_clusters': imap,
        'influence_map_all_clusters_inverse_kernels':
            with_inverse_kernel(imap)},
        args.warmup, args.runs)
    out['inverse'] = inv_facts
    lev = diag.influence_map(state, cohs, tile, bb, cluster=None, layout=lay)
    out['lev_min_max'] = [float(lev.min()), float(lev.max())]
    # coh in, lev out, and per (pair, chunk) the 8x8 block Hpq and the two
    # diagonal 4x4 sub-blocks of Hpp and of Hqq, all of it once
    nbytes = M * Rn * (32 + 8) + Nbase * M * K * (64 + 2 * 32) * 8
    ms = out['k_leverage']['ms_median']
    out.update(rows=Rn, clusters=M, chunks=M * K,
               bytes_k_leverage_must_move=nbytes,
               achieved_GB_per_s=round(nbytes / ms / 1e6, 1))
    return out


def shape_c(args):
    """One chunk per cluster: the 10 matrices of 512 that the leverage of
    single clusters inverts, from the same data as shape (b)."""
    T, M = 960, 10
    state, cohs, tile, bb = make(T, [1] * M)
    lay = hip_host.BaselineLayout(bb, tile.Nbase, T, 1, N, DEV)
    JtJ = torch.cat([
        ops.jtj_jtr(tile.x, cohs[ci], state.cluster_J(ci), bb, N, None,
                    None, 1, lay)[0] for ci in range(M)])
    fns, facts = inverse_paths(JtJ)
    out = compare(fns, args.warmup, args.runs)
    out['inverse'] = facts
    return out


def with_env(fn, *names):
    def run():
        os.environ.update({n: '1' for n in names})
        try:
            return fn()
        finally:
            for n in names:
                os.environ.pop(n)
    return run


def shape_d(args):
    """Shape (b) again for the float64 assembly of normal_f64.hip:
    ops.normal_matrices against the ten ops.jtj_jtr calls, what the inverse
    kernels flag for either matrix at mu = 1e-6, and the whole map with
    SAGECAL_NORMAL_F64=1 and SAGECAL_INVERSE_KERNEL=1, the latter alone, and
    neither."""
    T, M, K = 960, 10, 16
    state, cohs, tile, bb = make(T, [K] * M)
    Nbase, Rn = tile.Nbase, T * tile.Nbase
    lay = hip_host.BaselineLayout(bb, Nbase, T, 1, N, DEV)
    rows = R.chunk_rows_for(0, state.nchunks, T, Nbase, Rn, DEV)
    tab = ops.lbfgs_chunk_table(state.chunk_off, state.nchunks, T, DEV)
    pairs = ops.lbfgs_pair_table(bb, Nbase, DEV)

    def assemble32():
        return torch.cat([
            ops.jtj_jtr(tile.x, cohs[ci], state.cluster_J(ci), bb, N, None,
                        rows, K, lay)[0] for ci in range(M)])
    assemble64 = lambda: ops.normal_matrices(cohs, state.J, tab, pairs)
    imap = lambda: diag.influence_map(state, cohs, tile, bb, cluster=None,
                                      layout=lay)
    maps = {'influence_map_normal_f64_and_inverse_kernels': with_env(
                imap, 'SAGECAL_NORMAL_F64', 'SAGECAL_INVERSE_KERNEL'),
            'influence_map_inverse_kernels': with_env(
                imap, 'SAGECAL_INVERSE_KERNEL'),
            'influence_map_neither': imap}
    out = compare({'jtj_assembly_ten_calls_float32': assemble32,
                   'normal_matrices_float64': assemble64, **maps},
                  args.warmup, args.runs)
    J32, J64 = assemble32(), assemble64()
    flagged = lambda A: int(hip_host.spd_inverse_damped(
        A, 1e-6, return_info=True)[1].count_nonzero())
    out['kernels_flag_not_positive_definite_mu1e-06'] = {
        'float32_assembly': flagged(J32), 'float64_assembly': flagged(J64)}
    out['max_abs_float32_minus_float64_assembly'] = float(
        (J32 - J64).abs().max())
    out['max_abs_assembly'] = float(J64.abs().max())
    del J32, J64
    levs = {k: fn() for k, fn in maps.items()}
    names = list(levs)
    out['max_abs_diff_of_maps'] = {
        f'{a} vs {b}': float((levs[a] - levs[b]).abs().max())
        for i, a in enumerate(names) for b in names[i + 1:]}
    # coh in, the 40 doubles per (pair, piece) out and in again, JtJ out
    pieces = M * K * -(-(T // K) // hip_host.NORMAL_TSPLIT)
    nbytes = (M * Rn * 32 + 2 * pieces * Nbase * 40 * 8
              + M * K * (8 * N) ** 2 * 8)
    ms = out['normal_matrices_float64']['ms_median']
    out.update(rows=Rn, clusters=M, chunks=M * K,
               bytes_normal_matrices_must_move=nbytes,
               achieved_GB_per_s=round(nbytes / ms / 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/leverage.json')
    ap.add_argument('--sections', default='a_one_cluster_T8,b_bench_default')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    res = {'tool': 'tools/bench_leverage.py', 'warmup': args.warmup,
           'runs': args.runs, 'order': 'the paths of a shape in turn, '
           'repeated', 'device': 'MI355X (gfx950)', 'N': N}
    for name, fn in (('a_one_cluster_T8', shape_a),
                     ('b_bench_default', shape_b),
                     ('c_ten_chunks', shape_c),
                     ('d_normal_f64', shape_d)):
        if name not in args.sections.split(','):
            continue
        res[name] = fn(args)
        print(json.dumps({name: res[name]}), flush=True)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
