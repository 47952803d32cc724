"""Op dispatch: CUDA tensors -> the HIP/CDNA4 extension, CPU -> the PyTorch
reference implementation.

The HIP extension is MANDATORY on GPU: if a CUDA tensor reaches an op and
the extension is missing, we raise (no silent eager fallback — the driver's
round-end check verifies the native .so is actually loaded).
Set SAGECAL_FORCE_REFERENCE=1 to explicitly run the torch reference on GPU
(used only for kernel A/B numerics tests).
"""
import math
import os
import torch

from . import reference as R

_ext = None
_ext_err = None


def _load_ext():
    global _ext, _ext_err
    if _ext is not None or _ext_err is not None:
        return _ext
    try:
        import importlib
        _ext = importlib.import_module('sagecal_amd.ops.hip.dirac_hip')
    except Exception as e:  # noqa: BLE001
        _ext_err = e
        _ext = None
    return _ext


_token_counter = [0]


def obj_token(obj):
    """Stable per-object cache token. id() is NOT a safe cache key — CPython
    recycles addresses after GC, so an id()-keyed cache can serve STALE
    entries (seen in practice: sage._solve_group served a freed tile's
    coherency buffers). The token is stored on the object and dies with it."""
    tok = getattr(obj, '_sagecal_token', None)
    if tok is None:
        _token_counter[0] += 1
        tok = _token_counter[0]
        try:
            obj._sagecal_token = tok
        except AttributeError:   # __slots__/tensor subclass without attr
            return id(obj)
    return tok


def remember(cache, key, value, cap):
    """cache[key] = value in a dict bounded for long multi-MS runs: once it
    holds more than `cap` entries the oldest goes first. Returns value."""
    if len(cache) > cap:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


def have_ext():
    return _load_ext() is not None


def _use_hip(t):
    if not t.is_cuda:
        return False
    if os.environ.get('SAGECAL_FORCE_REFERENCE') == '1':
        return False
    if _load_ext() is None:
        raise RuntimeError(
            f"sagecal_amd HIP extension not available on GPU tensor "
            f"(build with python setup.py build_ext --inplace): {_ext_err}")
    return True


# ---------------------------------------------------------------------------

def predict_coh(pack, u, v, w, freq, freq0, fdelta, tdelta, dec0, **kw):
    if _use_hip(u):
        from . import hip_host
        return hip_host.predict_coh(pack, u, v, w, freq, freq0, fdelta,
                                    tdelta, dec0, **kw)
    return R.predict_coh(pack, u, v, w, freq, freq0, fdelta, tdelta, dec0,
                         **kw)


def _beamed_coh_reference(pack, u, v, w, fi, freq, freq0, fdelta, tdelta,
                          dec0, beam, ejones, pairs, Nbase):
    """One channel of the beamed all-channels predict off the GPU:
    beams.predict_coh_withbeam, the fp64 per-source yardstick, with row fi
    of the given gains [F, T, K, N] and/or patterns [F, T, K, 2, 2] (or
    [F, T, K, 1, 2, 2]; it knows one pattern per source only)."""
    from .. import beams
    if pairs is None:
        raise ValueError("beam and ejones need the station-pair table "
                         "`pairs`")
    Nbase = int(Nbase) or int(pairs.shape[0])
    T = int(u.shape[0]) // Nbase
    if ejones is not None and ejones.dim() == 6:
        if ejones.shape[3] != 1:
            raise ValueError("per-station E-Jones patterns are applied by "
                             "the GPU kernels only")
        ejones = ejones[:, :, :, 0]
    mode = 3 if beam is None else (1 if ejones is None else 2)
    bb = pairs[:Nbase].to(device=u.device, dtype=torch.long).repeat(T, 1)
    # gains and patterns are given, so config, times and geometry are unread
    return beams.predict_coh_withbeam(
        pack, u, v, w, freq, freq0, fdelta, tdelta, dec0, None, None, bb,
        Nbase, T, mode=mode, geom=(), gains=None if beam is None
        else beam[fi], ejones=None if ejones is None else ejones[fi])


def predict_coh_channels(pack, u, v, w, freqs, freq0, fdelta, tdelta, dec0,
                         reduce=None, beam=None, ejones=None, pairs=None,
                         Nbase=0, shapelets=False):
    """Coherencies of every channel of `freqs`, [F, M, R, 2, 2], or with
    reduce='mean' their mean over the channels [M, R, 2, 2]; fdelta is the
    width of one channel. Optional station beam per channel: `beam`
    [F, T, K, N] gains and/or `ejones` [F, T, K, NE, 2, 2] (or
    [F, T, K, 2, 2]) patterns, with `pairs` [Nbase, 2]. On the GPU one launch
    of the all-channels kernel, and with shapelets=True a second one for the
    pack's shapelet sources (without it they raise ValueError); elsewhere
    the per-channel loop over the fp64 reference, with a beam over
    beams.predict_coh_withbeam, which takes shapelet sources as they are
    and ignores `shapelets`."""
    if _use_hip(u):
        from . import hip_host
        return hip_host.predict_coh_channels(
            pack, u, v, w, freqs, freq0, fdelta, tdelta, dec0, reduce,
            beam=beam, ejones=ejones, pairs=pairs, Nbase=Nbase,
            shapelets=shapelets)
    if reduce not in (None, 'mean'):
        raise ValueError(f"reduce must be None or 'mean', got {reduce!r}")
    if beam is None and ejones is None:
        cohs = [R.predict_coh(pack, u, v, w, float(f), freq0, fdelta, tdelta,
                              dec0) for f in freqs]
    else:
        cohs = [_beamed_coh_reference(pack, u, v, w, fi, float(f), freq0,
                                      fdelta, tdelta, dec0, beam, ejones,
                                      pairs, Nbase)
                for fi, f in enumerate(freqs)]
    if not cohs:
        if reduce:
            raise ValueError("the mean over no channels is undefined")
        cd = torch.complex128 if u.dtype == torch.float64 \
            else torch.complex64
        return torch.empty((0, pack.M, u.shape[0], 2, 2), dtype=cd,
                           device=u.device)
    out = torch.stack(cohs)
    return out.mean(dim=0) if reduce else out


def residuals_multifreq(pack, x, u, v, w, freqs, freq0, fdelta, tdelta, dec0,
                        J, chunk_tab, pairs, subtract=None, beam=None,
                        ejones=None, shapelets=False):
    """x[f] - sum over clusters with subtract[ci] of J_p C_f J_q^H,
    [F, R, 2, 2], C_f with the station beam of `beam` [F, T, K, N] and/or
    `ejones` [F, T, K, NE, 2, 2] (or [F, T, K, 2, 2]) when given. J [Mt, N, 2, 2] packed solutions; chunk_tab [M, T] global
    chunk id per (cluster, timeslot); pairs [Nbase, 2], rows r = t*Nbase + b;
    a row whose pair has a negative entry keeps x. On the GPU one launch of
    the fused kernel, and with shapelets=True a second one for the pack's
    shapelet sources (without it they raise ValueError); elsewhere the
    per-channel loop over R.predict_coh (with a beam,
    beams.predict_coh_withbeam) and R.apply_jones, which ignores
    `shapelets`."""
    if _use_hip(u):
        from . import hip_host
        return hip_host.residuals_multifreq(
            pack, x, u, v, w, freqs, freq0, fdelta, tdelta, dec0, J,
            chunk_tab, pairs, subtract, beam=beam, ejones=ejones,
            shapelets=shapelets)
    T, Nbase = int(chunk_tab.shape[1]), int(pairs.shape[0])
    bb = pairs.to(device=x.device, dtype=torch.long).repeat(T, 1)
    ok = (bb >= 0).all(dim=1)
    bb = bb.clamp_min(0)
    rows = chunk_tab.to(device=x.device,
                        dtype=torch.long).repeat_interleave(Nbase, dim=1)
    out = torch.empty_like(x)
    for fi, f in enumerate(freqs):
        if beam is None and ejones is None:
            cohs = R.predict_coh(pack, u, v, w, float(f), freq0, fdelta,
                                 tdelta, dec0).to(x.dtype)
        else:
            cohs = _beamed_coh_reference(
                pack, u, v, w, fi, float(f), freq0, fdelta, tdelta, dec0,
                beam, ejones, pairs.clamp_min(0), 0).to(x.dtype)
        V = torch.zeros_like(cohs[0])
        for ci in range(cohs.shape[0]):
            if subtract is not None and not bool(subtract[ci]):
                continue
            V = V + R.apply_jones(cohs[ci], J, bb, rows[ci])
        out[fi] = torch.where(ok[:, None, None], x[fi] - V, x[fi])
    return out


def jtj_jtr(x, coh, J, bb, N, weights=None, chunk_rows=None, nchunk=1,
            layout=None):
    if _use_hip(x):
        from . import hip_host
        return hip_host.jtj_jtr(x, coh, J, bb, N, weights, chunk_rows,
                                nchunk, layout)
    return R.jtj_jtr(x, coh, J, bb, N, weights, chunk_rows, nchunk)


def apply_jones(coh, J, bb, chunk_rows=None, layout=None):
    if _use_hip(coh):
        from . import hip_host
        return hip_host.apply_jones(coh, J, bb, chunk_rows, layout)
    return R.apply_jones(coh, J, bb, chunk_rows)


def model_cost_per_chunk(x, coh, J, bb, N, weights=None, chunk_rows=None,
                         nchunk=1, layout=None):
    """Per-chunk weighted cost [nchunk] (kernel_fcost analog)."""
    if _use_hip(x) and layout is not None:
        from . import hip_host
        return hip_host.model_cost_per_chunk(x, coh, J, bb, N, weights,
                                             chunk_rows, nchunk, layout)
    V = R.apply_jones(coh, J, bb, chunk_rows)
    r = x - V
    e2 = (r.abs() ** 2).sum(dim=(-1, -2))
    if weights is not None:
        e2 = e2 * weights
    if chunk_rows is None:
        return e2.sum().unsqueeze(0)
    out = torch.zeros(nchunk, dtype=e2.dtype, device=e2.device)
    out.index_add_(0, chunk_rows, e2)
    return out


def model_and_cost(x, coh, J, bb, weights=None, chunk_rows=None):
    return R.model_and_cost(x, coh, J, bb, weights, chunk_rows)


def update_weights(r, nu, p=8):
    return R.update_weights(r, nu, p)


def update_nu_aecm(w, nu_old, **kw):
    return R.update_nu_aecm(w, nu_old, **kw)


def lbfgs_channels_on():
    """SAGECAL_LBFGS_CHANNELS=1 opts into the fused multi-channel LBFGS
    kernels (lbfgs_cost_grad_channels) wherever a device cost/gradient is
    evaluated; off by default, and SAGECAL_FORCE_REFERENCE=1 overrides
    it."""
    return (os.environ.get('SAGECAL_LBFGS_CHANNELS') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


_lbfgs_tab_memo = {}   # chunk tables and pair tables of lbfgs_cost_grad


def _memo(key, build):
    hit = _lbfgs_tab_memo.get(key)
    if hit is None:
        hit = remember(_lbfgs_tab_memo, key, build(), 64)
    return hit


def lbfgs_chunk_table(chunk_off, nchunks, T, device):
    """[M, T] int32 on `device`: chunk_off[ci] + R.chunk_rows_for per
    timeslot, the table lbfgs_cost_grad_channels takes; one tensor per
    (nchunks, chunk_off, T, device)."""
    nchunks = [int(n) for n in nchunks]
    chunk_off = [int(o) for o in chunk_off]

    def build():
        rows = []
        for ci, off in enumerate(chunk_off):
            r = R.chunk_rows_for(ci, nchunks, T, 1, T, 'cpu')
            if r is None:
                r = torch.zeros(T, dtype=torch.long)
            rows.append(r + off)
        return torch.stack(rows).to(device=device, dtype=torch.int32)
    return _memo((tuple(nchunks), tuple(chunk_off), T, str(device)), build)


def lbfgs_pair_table(bb, Nbase, device):
    """bb[:Nbase] as the int32 pair table on `device`, one tensor per bb
    tensor: the kernels' index tables are remembered per pair table."""
    build = lambda: bb[:Nbase].to(device=device,
                                  dtype=torch.int32).contiguous()
    try:
        return _memo((obj_token(bb), bb._version, Nbase, str(device)), build)
    except RuntimeError:                 # inference tensor: no version
        return build()


def lbfgs_cost_grad_channels(xs, cohs, J, chunk_tab, pairs, robust_nu=None):
    """(cost, grad [Mt*N*8]) of the LBFGS objective over all channels: the
    sum over f of lbfgs_cost_grad(xs[f], cohs[f], ...) with xs [F, R, 2, 2],
    cohs [F, M, R, 2, 2], J [Mt, N, 2, 2], chunk_tab [M, T] global chunk id
    per (cluster, timeslot), pairs [Nbase, 2], rows r = t*Nbase + b; a row
    whose pair has a negative entry adds nothing. On the GPU three launches
    of the kernels of lbfgs_mf.hip; elsewhere that sum over
    R.lbfgs_cost_grad, in the input precision."""
    if _use_hip(xs):
        from . import hip_host
        return hip_host.lbfgs_cost_grad_channels(xs, cohs, J, chunk_tab,
                                                 pairs, robust_nu)
    F, Rn = int(xs.shape[0]), int(xs.shape[1])
    M, T, Nbase = int(cohs.shape[1]), int(chunk_tab.shape[1]), \
        int(pairs.shape[0])
    if tuple(cohs.shape) != (F, M, Rn, 2, 2) or chunk_tab.shape[0] != M \
            or T * Nbase != Rn:
        raise ValueError("xs [F, R, 2, 2], cohs [F, M, R, 2, 2], chunk_tab "
                         "[M, T] and pairs [Nbase, 2] with T * Nbase rows")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    bb = pairs.to(device=xs.device, dtype=torch.long).repeat(T, 1)
    live = (bb >= 0).all(dim=1)[:, None, None]
    bb = bb.clamp_min(0)        # flagged rows get x = coh = 0: res = 0
    # R.lbfgs_cost_grad with one chunk per (cluster, timeslot): chunk
    # ci*T + t holds J[chunk_tab[ci, t]], whatever the table looks like
    tab = chunk_tab.to(device=xs.device, dtype=torch.long).reshape(-1)
    Jt = J[tab]
    chunk_off, nchunks = [ci * T for ci in range(M)], [T] * M
    cost = xs.real.new_zeros(())
    grad = xs.real.new_zeros(Mt, N * 8)
    zero = xs.new_zeros(())
    for f in range(F):
        c, g = R.lbfgs_cost_grad(
            torch.where(live, xs[f], zero), torch.where(live, cohs[f], zero),
            Jt, chunk_off, nchunks, bb, T, Nbase, robust_nu)
        cost = cost + c
        grad.index_add_(0, tab, g.reshape(M * T, N * 8))
    return cost, grad.reshape(-1)


def joint_kernel_on():
    """SAGECAL_JOINT_KERNEL=1 opts lm.joint_lm_solve into the kernels of
    joint_jtj.hip on device tensors; off by default, and
    SAGECAL_FORCE_REFERENCE=1 overrides it."""
    return (os.environ.get('SAGECAL_JOINT_KERNEL') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


def rtr_kernel_on():
    """SAGECAL_RTR_KERNEL=1 opts rtr.rtr_solve and rtr.rtr_solve_graphed
    into the one-launch inner solve of rtr_tcg.hip on device tensors; off by
    default, and SAGECAL_FORCE_REFERENCE=1 overrides it."""
    return (os.environ.get('SAGECAL_RTR_KERNEL') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


def chol_blocked_on():
    """SAGECAL_CHOL_BLOCKED=1 opts hip_host.chol_solve_damped, and with it
    lm.joint_lm_solve, into the blocked kernels of cholesky_blocked.hip for
    n > 4096 (up to 16384); off by default, and SAGECAL_FORCE_REFERENCE=1
    overrides it."""
    return (os.environ.get('SAGECAL_CHOL_BLOCKED') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


def inverse_kernel_on():
    """SAGECAL_INVERSE_KERNEL=1 opts diagnostics.leverage and
    diagnostics.influence_map into the float64 inverse kernels of
    spd_inverse.hip on device tensors; off by default, and
    SAGECAL_FORCE_REFERENCE=1 overrides it."""
    return (os.environ.get('SAGECAL_INVERSE_KERNEL') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


INVERSE_SPLIT_ENTRIES = 1 << 23   # most matrix entries of one linalg.inv call
INVERSE_KERNEL_MAXN = 1024        # SPD_INVERSE_MAXN of launchers.h


def spd_inverse_torch(JtJ, mu):
    """inv(JtJ + mu I) per matrix, in float64, by torch.linalg.inv. Batches
    of at most 2^23 matrix entries (32 chunks of 64 stations) go to it at a
    time: on the MI355X its batched triangular solve ran out of workspace
    and raised for 160 matrices of 512, while 4 to 64 at a time all gave the
    same bits in the same 0.31 to 0.34 s."""
    n = JtJ.shape[-1]
    if torch.is_tensor(mu):
        mu = mu.to(device=JtJ.device, dtype=torch.float64).reshape(-1, 1, 1)
    A = JtJ.to(torch.float64) + mu * torch.eye(n, dtype=torch.float64,
                                               device=JtJ.device)
    step = max(1, INVERSE_SPLIT_ENTRIES // (n * n))
    if A.shape[0] <= step:
        return torch.linalg.inv(A)
    return torch.cat([torch.linalg.inv(A[i:i + step])
                      for i in range(0, A.shape[0], step)])


def spd_inverse_damped(JtJ, mu):
    """X [Mt, n, n] float64 = (JtJ + mu I)^-1 for symmetric positive
    definite JtJ + mu I: JtJ [Mt, n, n] float32 or float64, mu a number or a
    tensor of one value or one per matrix. On the GPU, for n a multiple of 8
    in 8..1024, the kernels of spd_inverse.hip (blocked Cholesky, inverse of
    the factor and its product with itself, in float64 on the matrix unit):
    they read the lower triangle of JtJ, return X == X^T to the bit, the
    same bits from call to call and in any batch, and all NaN for a matrix
    that is not positive definite. Elsewhere, and for other n,
    spd_inverse_torch, which raises for a singular matrix."""
    n = int(JtJ.shape[-1])
    if _use_hip(JtJ) and JtJ.dim() == 3 and JtJ.shape[0] >= 1 \
            and n % 8 == 0 and 8 <= n <= INVERSE_KERNEL_MAXN \
            and JtJ.dtype in (torch.float32, torch.float64):
        from . import hip_host
        return hip_host.spd_inverse_damped(JtJ, mu)
    return spd_inverse_torch(JtJ, mu)


def rtr_tcg(JtJ, Jtr, J, iw, delta, maxit=12, kappa=0.01):
    """The inner solve of one RTR outer iteration at J [n, N, 2, 2], from
    the normal equations JtJ [n, 8N, 8N], Jtr [n, 8N] in reference.vecR
    order, the station scale iw [N] and the radius delta [n]: returns
    (g, eta, Heta, stats) with g the Riemannian gradient, eta the truncated-CG
    step, Heta = hess_vec(J, eta), each [n, N, 2, 2], and stats [n, 4] =
    (<g,g>, <g,eta>, <eta,Heta>, CG iterations entered) in the metric
    2 Re tr(a^H b). On the GPU one launch of k_rtr_tcg (rtr_tcg.hip), in
    float32; elsewhere the torch code of solvers.rtr in the input
    precision."""
    if _use_hip(J):
        from . import hip_host
        return hip_host.rtr_tcg(JtJ, Jtr, J, iw, delta, maxit, kappa)
    from ..solvers import rtr
    obj = rtr._Objective(None, iw)
    obj.JtJ, obj.Jtr = JtJ, Jtr
    g = obj.grad(J)
    eta, nit = rtr._tcg_fixed(obj, J, g, delta, maxit, kappa, count=True)
    Heta = obj.hess_vec(J, eta)
    stats = torch.stack([rtr._inner(g, g), rtr._inner(g, eta),
                         rtr._inner(eta, Heta), nit], dim=-1)
    return g, eta, Heta, stats


def leverage_rows(cohs, J, Hinv, chunk_tab, pairs, weights=None):
    """Leverage lev [M, R] float64 of every visibility row in every
    cluster's solve: with (p, q) = pairs[b], c = chunk_tab[ci, t] and row
    r = t*Nbase + b, G1 = C J_q^H, K = J_p C, D1 = diagnostics._lin_blocks(G1)
    and D2 = diagnostics._anti_blocks(K),
      lev[ci, r] = tr(D1 Hpp D1^T) + tr(D2 Hqq D2^T) + 2 tr(D1 Hpq D2^T)
    with Hxy the 8x8 block of Hinv[c] at stations (x, y), times weights[r]
    when given. cohs [M, R, 2, 2], J [Mt, N, 2, 2], Hinv [Mt, 8N, 8N],
    chunk_tab [M, T] global chunk ids, pairs [Nbase, 2], R = T * Nbase; a row
    whose pair has a negative entry gets 0. On the GPU one launch of
    k_leverage (leverage.hip) in float64 on complex64 inputs; elsewhere this
    formula in torch on complex128 upcasts, cluster by cluster, with the
    blocks of Hinv taken per (chunk, pair)."""
    if _use_hip(cohs):
        from . import hip_host
        return hip_host.leverage_rows(cohs, J, Hinv, chunk_tab, pairs,
                                      weights)
    from ..solvers import diagnostics as diag
    M, Rn = int(cohs.shape[0]), int(cohs.shape[1])
    T, Nbase = int(chunk_tab.shape[1]), int(pairs.shape[0])
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if tuple(cohs.shape) != (M, Rn, 2, 2) or chunk_tab.shape[0] != M \
            or T * Nbase != Rn or tuple(Hinv.shape) != (Mt, 8 * N, 8 * N):
        raise ValueError("cohs [M, R, 2, 2], Hinv [Mt, 8N, 8N], chunk_tab "
                         "[M, T] and pairs [Nbase, 2] with T * Nbase rows")
    dev = cohs.device
    pr = pairs.to(device=dev, dtype=torch.long)
    live = (pr >= 0).all(dim=1)
    p, q = pr.clamp_min(0).unbind(1)
    Jd = J.to(torch.complex128)
    H5 = Hinv.to(torch.float64).reshape(Mt, N, 8, N, 8)
    lev = torch.zeros(M, T, Nbase, dtype=torch.float64, device=dev)
    for ci in range(M):
        ct = chunk_tab[ci].to(device=dev, dtype=torch.long)
        cs, slot = torch.unique(ct, return_inverse=True)
        c2 = cs[:, None]
        # [chunks of ci, Nbase, 8, 8], then per timeslot
        Hpp, Hqq, Hpq = (H5[c2, a[None], :, b[None], :][slot]
                         for a, b in ((p, p), (q, q), (p, q)))
        C = cohs[ci].to(torch.complex128).reshape(T, Nbase, 2, 2)
        G1 = C @ Jd[ct][:, q].conj().transpose(-1, -2)
        K = Jd[ct][:, p] @ C
        D1 = diag._lin_blocks(G1.reshape(-1, 2, 2)).reshape(T, Nbase, 8, 8)
        D2 = diag._anti_blocks(K.reshape(-1, 2, 2)).reshape(T, Nbase, 8, 8)
        D1t, D2t = D1.transpose(-1, -2), D2.transpose(-1, -2)
        lev[ci] = (D1 @ Hpp @ D1t + D2 @ Hqq @ D2t
                   + 2 * (D1 @ Hpq @ D2t)).diagonal(dim1=-2, dim2=-1).sum(-1)
    lev = torch.where(live[None, None, :], lev, lev.new_zeros(()))
    lev = lev.reshape(M, Rn)
    if weights is not None:
        lev = lev * weights.to(device=dev, dtype=torch.float64)
    return lev


def normal_f64_on():
    """SAGECAL_NORMAL_F64=1 opts diagnostics.leverage and
    diagnostics.influence_map into the float64 normal matrices of
    normal_f64.hip on device tensors with structured rows; off by default,
    and SAGECAL_FORCE_REFERENCE=1 overrides it."""
    return (os.environ.get('SAGECAL_NORMAL_F64') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


def normal_matrices(cohs, J, chunk_tab, pairs, weights=None):
    """JtJ [Mt, 8N, 8N] float64, the Gauss-Newton normal matrix of every
    chunk of every cluster: with (p, q) = pairs[b], c = chunk_tab[ci, t] and
    row r = t*Nbase + b, G1 = C J_q^H, K = J_p C, D1 =
    diagnostics._lin_blocks(G1) and D2 = diagnostics._anti_blocks(K),
      JtJ[c] = sum over the rows of c of weights[r] [D1 D2]^T [D1 D2]
    scattered to stations (p, q) in reference.vecR order, what
    reference.jtj_jtr assembles; it does not depend on the data. cohs
    [M, R, 2, 2], J [Mt, N, 2, 2], chunk_tab [M, T] global chunk ids, pairs
    [Nbase, 2], R = T * Nbase, weights [R] or None; a pair with a negative
    entry adds nothing. On the GPU the two kernels of normal_f64.hip, in
    float64 on complex64 inputs (each pair at most once in the table);
    elsewhere reference.jtj_jtr on complex128 upcasts, cluster by cluster."""
    if _use_hip(cohs):
        from . import hip_host
        return hip_host.normal_matrices(cohs, J, chunk_tab, pairs, weights)
    if cohs.dim() != 4 or J.dim() != 4 or chunk_tab.dim() != 2 \
            or pairs.dim() != 2:
        raise ValueError("cohs [M, R, 2, 2], J [Mt, N, 2, 2], chunk_tab "
                         "[M, T] and pairs [Nbase, 2]")
    M, Rn = int(cohs.shape[0]), int(cohs.shape[1])
    T, Nbase = int(chunk_tab.shape[1]), int(pairs.shape[0])
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if tuple(cohs.shape) != (M, Rn, 2, 2) or chunk_tab.shape[0] != M \
            or T * Nbase != Rn or tuple(pairs.shape) != (Nbase, 2) \
            or (weights is not None and tuple(weights.shape) != (Rn,)):
        raise ValueError("cohs [M, R, 2, 2], chunk_tab [M, T], pairs "
                         "[Nbase, 2] and weights [R] with T * Nbase rows")
    dev = cohs.device
    pr = pairs.to(device=dev, dtype=torch.long)
    live = (pr >= 0).all(dim=1).repeat(T)
    bb = pr.clamp_min(0).repeat(T, 1)
    Jd = J.to(torch.complex128)
    wt = None if weights is None else weights.to(device=dev,
                                                 dtype=torch.float64)
    JtJ = torch.zeros(Mt, 8 * N, 8 * N, dtype=torch.float64, device=dev)
    for ci in range(M):
        ct = chunk_tab[ci].to(device=dev, dtype=torch.long)
        cs, slot = torch.unique(ct, return_inverse=True)
        C = cohs[ci].to(torch.complex128)
        C = torch.where(live[:, None, None], C, C.new_zeros(()))
        JtJ[cs] += R.jtj_jtr(C, C, Jd[cs], bb, N, wt,
                             slot.repeat_interleave(Nbase), len(cs))[0]
    return JtJ


def diffuse_kernel_on():
    """SAGECAL_DIFFUSE_KERNEL=1 opts ConsensusADMM.diffuse_coherencies, the
    diffuse hook of sagecal-mpi -D, into the kernels of diffuse.hip on device
    tensors; off by default, and SAGECAL_FORCE_REFERENCE=1 overrides it."""
    return (os.environ.get('SAGECAL_DIFFUSE_KERNEL') == '1'
            and os.environ.get('SAGECAL_FORCE_REFERENCE') != '1')


DIFFUSE_KERNEL_MAX_GZ = 4     # DIFFUSE_MAX_GZ and DIFFUSE_MAX_N2 of launchers.h
DIFFUSE_KERNEL_MAX_N2 = 32


def diffuse_coherencies(u, v, w, pairs, T, Z, beta_z, Cm, beta_c, lmn, freq,
                        fdelta):
    """Coherencies V [T * Nbase, 2, 2] of a diffuse shapelet cluster with the
    per-station spatial model applied, shapelet.recalculate_diffuse_
    coherencies on structured rows: with (p, q) = pairs[b], row r = t*Nbase
    + b, n1 = Gc + Gz - 1, n2 = Gz + n1 - 1, g1 = product_scale(beta_c,
    beta_z) and g2 = product_scale(beta_z, g1),
      H_pq = Z_p x (C x Z_q^H)     (Jones series products, n2 x n2 modes)
      V_r = 2 pi sum_kl basis_kl(-u_r f, v_r f; g2) H_pq[k,l]
            * exp(i 2 pi f (u_r l + v_r m + w_r (n-1)))
            * |sinc(pi fdelta (u_r l + v_r m + w_r (n-1)))|
    u, v, w [T * Nbase] in seconds, pairs [Nbase, 2] (the table of
    lbfgs_pair_table), Z [N, Gz*Gz, 2, 2] at scale beta_z, Cm [Gc*Gc, 2, 2]
    at scale beta_c, lmn = (l, m, n - 1) of the cluster, freq and fdelta in
    Hz; a row whose pair has a negative entry gets zeros. On the GPU, for
    Gz <= 4 and n2 <= 32, the two kernels of diffuse.hip: series products in
    float64 on the matrix unit, the mode sum in float32, complex64 out, the
    same bits from call to call. Elsewhere, and for larger series, the host
    function in complex128 on rows expanded from the table, its result
    moved to the device of u."""
    Gz, Gc = math.isqrt(Z.shape[1]), math.isqrt(Cm.shape[0])
    Nbase = int(pairs.shape[0])
    if tuple(u.shape) != (int(T) * Nbase,):
        raise ValueError(f"u must be [T * Nbase] = [{int(T) * Nbase}], got "
                         f"{tuple(u.shape)}")
    if _use_hip(u) and Gz <= DIFFUSE_KERNEL_MAX_GZ \
            and Gc + 2 * Gz - 2 <= DIFFUSE_KERNEL_MAX_N2:
        from . import hip_host
        return hip_host.diffuse_coherencies(u, v, w, pairs, T, Z, beta_z, Cm,
                                            beta_c, lmn, freq, fdelta)
    from .. import shapelet
    pr = pairs.to(device='cpu', dtype=torch.long)
    live = (pr >= 0).all(dim=1).repeat(int(T))
    f64 = lambda t: t.to(device='cpu', dtype=torch.float64)
    out = shapelet.recalculate_diffuse_coherencies(
        f64(u), f64(v), f64(w), pr.clamp_min(0).repeat(int(T), 1), Z.cpu(),
        beta_z, Cm.cpu(), beta_c, *lmn, freq, fdelta)
    out = torch.where(live[:, None, None], out, out.new_zeros(()))
    return out.to(u.device)


def _joint_blocks(chunk_off, nchunks, blocked):
    """Chunks per cluster Kb of the blocked layout, or None for dense."""
    if not blocked:
        return None
    nchunks = [int(n) for n in nchunks]
    Kb = nchunks[0]
    if any(n != Kb for n in nchunks) or \
            [int(o) for o in chunk_off] != [ci * Kb
                                            for ci in range(len(nchunks))]:
        raise ValueError("blocked=True needs the same chunk count in every "
                         f"cluster, packed in cluster order; got {nchunks}")
    return Kb


def joint_jtj_jtr(x, cohs, J, chunk_off, nchunks, bb, T, Nbase, weights=None,
                  blocked=False):
    """(H, g, cost) of the joint cross-cluster Gauss-Newton step,
    R.joint_jtj_jtr: H [P, P], g [P], cost [] with P = 8 Mt N, parameter
    order (chunk, station, 8). blocked=True, for the same chunk count Kb in
    every cluster (else ValueError): chunk k of every cluster covers the
    same timeslots and the blocks do not couple, so only they are returned,
    H [Kb, Pb, Pb], g [Kb, Pb], cost [Kb] with Pb = 8 M N and parameter order
    (cluster, station, 8). On the GPU the two launches of joint_jtj.hip, in
    float32, where rows r = t*Nbase + b and a pair of bb[:Nbase] with a
    negative entry adds nothing; elsewhere R.joint_jtj_jtr and, blocked, a
    gather of its diagonal blocks."""
    Kb = _joint_blocks(chunk_off, nchunks, blocked)
    if _use_hip(x):
        from . import hip_host
        return hip_host.joint_jtj_jtr(
            x, cohs, J, lbfgs_chunk_table(chunk_off, nchunks, T, x.device),
            lbfgs_pair_table(bb, Nbase, x.device), weights, blocked)
    H, g, _ = R.joint_jtj_jtr(x, cohs, J, chunk_off, nchunks, bb, T, Nbase,
                              weights)
    if not blocked:
        return H, g, _
    M, N = len(nchunks), int(J.shape[1])
    # parameter (k; ci, s, i) of block k sits at ((ci*Kb + k)*N + s)*8 + i
    idx = ((torch.arange(M, device=x.device)[None, :, None] * Kb
            + torch.arange(Kb, device=x.device)[:, None, None]) * (N * 8)
           + torch.arange(N * 8, device=x.device)[None, None, :]
           ).reshape(Kb, -1)
    Hb = H[idx[:, :, None], idx[:, None, :]]
    return Hb, g[idx], joint_cost(x, cohs, J, chunk_off, nchunks, bb, T,
                                  Nbase, weights, blocked=True)


def joint_cost(x, cohs, J, chunk_off, nchunks, bb, T, Nbase, weights=None,
               blocked=False):
    """The weighted cost of joint_jtj_jtr alone at J, [] or with
    blocked=True per block [Kb]: the trial cost of the joint LM. On the GPU
    the cost kernels of joint_jtj.hip, which allocate no H."""
    Kb = _joint_blocks(chunk_off, nchunks, blocked)
    if _use_hip(x):
        from . import hip_host
        return hip_host.joint_cost(
            x, cohs, J, lbfgs_chunk_table(chunk_off, nchunks, T, x.device),
            lbfgs_pair_table(bb, Nbase, x.device), weights, blocked)
    V = torch.zeros_like(x)
    for ci in range(len(nchunks)):
        rows = R.chunk_rows_for(ci, nchunks, T, Nbase, x.shape[0], x.device)
        V = V + R.apply_jones(
            cohs[ci], J[chunk_off[ci]:chunk_off[ci] + int(nchunks[ci])], bb,
            rows)
    e2 = ((x - V).abs() ** 2).sum(dim=(-1, -2))
    if weights is not None:
        e2 = e2 * weights
    if not blocked:
        return e2.sum()
    rows = R.chunk_rows_for(0, nchunks, T, Nbase, x.shape[0], x.device)
    if rows is None:
        return e2.sum().unsqueeze(0)
    return torch.zeros(Kb, dtype=e2.dtype, device=e2.device).index_add_(
        0, rows, e2)


def lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks, bb, T, Nbase,
                    robust_nu=None, weights=None):
    if _use_hip(x) and lbfgs_channels_on() and weights is None \
            and x.shape[0] == T * Nbase:
        return lbfgs_cost_grad_channels(
            x[None], cohs[None], J_packed,
            lbfgs_chunk_table(chunk_off, nchunks, T, x.device),
            lbfgs_pair_table(bb, Nbase, x.device), robust_nu)
    if _use_hip(x):
        from . import hip_host
        return hip_host.lbfgs_cost_grad(x, cohs, J_packed, chunk_off,
                                        nchunks, bb, T, Nbase, robust_nu,
                                        weights)
    return R.lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks, bb, T,
                             Nbase, robust_nu, weights)
