"""Batched Levenberg-Marquardt on per-station Jones matrices.

Re-implements the solver semantics of
/root/reference/src/lib/Dirac/clmfit.c (clevmar_der_single_nocuda: mu
damping schedule, rho accept/reject, eps1/eps2/eps3 termination) and
robustlm.c (IRLS Student's-t outer loop), re-architected MI355X-first:
instead of one 8N-parameter solve at a time on a 2-GPU pthread pipeline
(lmfit_cuda.c:451-575), ALL problems (cluster x time-chunk) iterate together
as one batched solver — one fused JtJ/Jtr kernel launch + one batched
Cholesky per LM iteration, sized so a 256-CU GPU is actually filled.

Ordered-subsets (OS-LM, oslmfit.c) acceleration: each outer pass runs LM on
a random contiguous fraction of the baselines then a final full pass.
"""
import os
import torch

from ..ops import dispatch as ops

# hipGraph cache for the fixed-iteration LM body: keyed by problem shape.
# Capturing the whole inner loop removes all per-iteration host dispatch
# (the loop is host-sync-free by construction).
_lm_graph_cache = {}


class LMProblem:
    """One batched LM problem set: for a fixed cluster, all its time-chunks
    (or for SAGE-batched mode: all clusters x chunks concatenated)."""

    def __init__(self, x, coh, bb, N, nchunk=1, chunk_rows=None,
                 weights=None, layout=None, admm=None):
        self.x = x              # [B,2,2] complex (data with own model added)
        self.coh = coh          # [B,2,2] complex cluster coherency
        self.bb = bb            # [B,2] long
        self.N = N
        self.nchunk = nchunk
        self.chunk_rows = chunk_rows  # [B] long or None
        self.weights = weights  # [B] float or None
        self.layout = layout    # BaselineLayout (GPU kernels) or None
        # consensus-ADMM augmentation (rtr_solve_robust_admm.c analog for
        # LM): admm = (rho [nchunk], Y [nchunk,N,2,2], BZ [nchunk,N,2,2]);
        # adds  y^T(J - BZ) + rho/2 ||J - BZ||^2  to the cost.
        self.admm = admm


def lm_solve(prob, J0, maxiter=30, tau=1e-3, eps1=1e-9, eps2=1e-9,
             verbose=False):
    if (prob.layout is not None and prob.x.is_cuda
            and os.environ.get('SAGECAL_NO_GRAPH') != '1'):
        # run the fixed-iteration graph in segments of 4 with a cheap
        # convergence poll between: late EM sweeps often converge in a few
        # iterations and the remaining replays are wasted work
        seg = 4 if maxiter > 4 else maxiter
        J = J0
        info = None
        done = 0
        cost_prev = None
        while done < maxiter:
            n = min(seg, maxiter - done)
            J, info = _lm_solve_graphed(prob, J, n, tau, eps1, eps2)
            done += n
            c = float(info['final_cost'].sum())
            if (cost_prev is not None
                    and abs(cost_prev - c) < 1e-4 * abs(cost_prev)):
                break
            cost_prev = c
        return J, info
    return _lm_solve_eager(prob, J0, maxiter, tau, eps1, eps2)


def _lm_solve_eager(prob, J0, maxiter=30, tau=1e-3, eps1=1e-9, eps2=1e-9,
                    verbose=False):
    """Batched LM: J0 [nchunk, N, 2, 2] complex initial Jones.

    Returns (J, info dict). All chunks iterate in lockstep with per-chunk
    damping/accept state. The whole iteration is host-sync-free (tensor
    masks for accept/reject, cholesky_ex instead of throwing cholesky);
    convergence is only polled every 8 iterations so the GPU pipeline
    stays full (the reference's per-iteration termination checks are a
    CPU-ism).

    Math follows clmfit.c:240-420: mu = tau*max(diag(JtJ)) init; accept step
    if rho>0 with mu *= max(1/3, 1-(2rho-1)^3), nu=2; else mu *= nu, nu *= 2.
    """
    x, coh, bb, N = prob.x, prob.coh, prob.bb, prob.N
    nchunk = prob.nchunk
    dev = x.device
    rdt = x.real.dtype
    J = J0.clone()
    nu = torch.full((nchunk,), 2.0, dtype=rdt, device=dev)
    active = torch.ones(nchunk, dtype=torch.bool, device=dev)

    JtJ, Jtr, _ = ops.jtj_jtr(x, coh, J, bb, N, prob.weights,
                              prob.chunk_rows, nchunk, prob.layout)
    JtJ, Jtr = _apply_admm_terms(JtJ, Jtr, J, prob, N, nchunk)
    cost = _total_cost(x, coh, J, bb, prob)
    init_cost = cost.clone()
    eye = torch.eye(8 * N, dtype=rdt, device=dev).unsqueeze(0)
    diag_max = JtJ.diagonal(dim1=-2, dim2=-1).max(dim=-1).values
    mu = tau * diag_max
    niter = 0
    # mw Cholesky handles up to n=4096 (chunked panels,
    # k_cholmw_panel_big) — hardware-validated end of round 2
    # (profiles/standalone_validate_r2.txt); SAGECAL_CHOL_BIG=0 opts out
    chol_cap = 1024 if os.environ.get('SAGECAL_CHOL_BIG') == '0' else 4096
    use_hip_chol = (prob.layout is not None and x.is_cuda
                    and 8 * N <= chol_cap)
    for it in range(maxiter):
        niter = it + 1
        if use_hip_chol:
            from ..ops.hip_host import chol_solve_damped
            dp = chol_solve_damped(JtJ, Jtr, mu)
        else:
            A = JtJ + mu[:, None, None] * eye
            dp = _chol_solve(A, Jtr)
        dp = torch.nan_to_num(dp, nan=0.0, posinf=0.0, neginf=0.0)
        dpc = _vec_to_jones(dp, nchunk, N)
        Jnew = J + dpc
        cost_new = _total_cost(x, coh, Jnew, bb, prob)
        denom = (dp * (mu[:, None] * dp + Jtr)).sum(dim=-1).clamp_min(1e-30)
        rho = (cost - cost_new) / denom
        accept = (rho > 0) & active
        stepn = dp.norm(dim=-1)
        pnorm = _jones_norm(J, nchunk)
        small = stepn < eps2 * (pnorm + eps2)
        J = torch.where(accept[:, None, None, None], Jnew, J)
        cost = torch.where(accept, cost_new, cost)
        fac = (1.0 - (2.0 * rho - 1.0) ** 3).clamp_min(1.0 / 3.0)
        mu = torch.where(accept, mu * fac, mu)
        nu = torch.where(accept, torch.full_like(nu, 2.0), nu)
        reject = (~accept) & active
        mu = torch.where(reject, mu * nu, mu)
        nu = torch.where(reject, nu * 2.0, nu)
        active = active & ~small
        if it + 1 < maxiter:
            # recompute JtJ/Jtr at (possibly) new J
            JtJ, Jtr, _ = ops.jtj_jtr(x, coh, J, bb, N, prob.weights,
                                      prob.chunk_rows, nchunk, prob.layout)
            JtJ, Jtr = _apply_admm_terms(JtJ, Jtr, J, prob, N, nchunk)
            gnorm = Jtr.abs().max(dim=-1).values
            active = active & (gnorm > eps1)
            if (it & 7) == 7 and not bool(active.any()):
                break
    info = {'init_cost': init_cost, 'final_cost': cost, 'niter': niter}
    return J, info


def _apply_admm_terms(JtJ, Jtr, J, prob, N, nchunk):
    """Add the consensus augmentation to the normal equations:
    JtJ += rho/2 I;  Jtr -= vecR(Y/2 + rho/2 (J - BZ))."""
    if prob.admm is None:
        return JtJ, Jtr
    rho, Y, BZ = prob.admm
    rho = rho.to(JtJ.dtype)
    JtJ = JtJ + (0.5 * rho)[:, None, None] * torch.eye(
        8 * N, dtype=JtJ.dtype, device=JtJ.device).unsqueeze(0)
    extra = 0.5 * Y + (0.5 * rho)[:, None, None, None] * (J - BZ)
    from ..ops.reference import vecR
    Jtr = Jtr - vecR(extra).reshape(nchunk, 8 * N).to(Jtr.dtype)
    return JtJ, Jtr


def _admm_cost(J, prob):
    """Per-chunk  Re<Y, J-BZ> + rho/2 ||J-BZ||^2."""
    rho, Y, BZ = prob.admm
    d = J - BZ
    lin = (Y.conj() * d).real.sum(dim=(-1, -2, -3))
    quad = 0.5 * rho * (d.abs() ** 2).sum(dim=(-1, -2, -3))
    return (lin + quad).to(torch.float32 if J.dtype == torch.complex64
                           else torch.float64)


def _total_cost(x, coh, J, bb, prob):
    c = _per_chunk_cost(x, coh, J, bb, prob)
    if prob.admm is not None:
        c = c + _admm_cost(J, prob).to(c.dtype)
    return c


def _chol_solve(A, b):
    """Batched SPD solve via cholesky_ex (no host sync, no throw); a failed
    factorization yields NaNs in that chunk's step, which the LM
    accept/reject mask rejects (mu grows and the next A is better
    conditioned) — self-healing without synchronization."""
    L, info = torch.linalg.cholesky_ex(A)
    return torch.cholesky_solve(b.unsqueeze(-1), L).squeeze(-1)


def _vec_to_jones(dp, nchunk, N):
    """Real [nchunk, 8N] -> complex [nchunk, N, 2, 2] (row-major interleaved
    re/im order, matching ops.reference.vecR)."""
    return torch.view_as_complex(
        dp.reshape(nchunk, N, 2, 2, 2).contiguous())


def _jones_norm(J, nchunk):
    return torch.view_as_real(J).reshape(nchunk, -1).norm(dim=-1)


def _per_chunk_cost(x, coh, J, bb, prob):
    """Weighted residual cost per chunk [nchunk]."""
    return ops.model_cost_per_chunk(x, coh, J, bb, prob.N, prob.weights,
                                    prob.chunk_rows, prob.nchunk,
                                    prob.layout)


def os_lm_solve(prob, J0, maxiter=30, nsubsets=4, seed=0, **kw):
    """Ordered-subsets LM (oslmfit.c / oslevmar_der_single_*): a few LM
    iterations on each subset — visited in random ORDER, like the
    reference's random_permutation over subsets (lmfit.c:1084) — then a
    final pass on the full data.

    Subsets are contiguous WHOLE-TIMESLOT ranges, identical across the
    seg axis, so the seg*(T*Nbase)+t*Nbase+b row structure survives and
    the GPU kernels stay on the structured (BaselineLayout + hipGraph)
    path instead of falling back to eager."""
    B = prob.x.shape[0]
    dev = prob.x.device
    g = torch.Generator(device='cpu').manual_seed(seed)
    iters_per = max(2, maxiter // (nsubsets + 1))
    order = torch.randperm(nsubsets, generator=g).tolist()
    J = J0
    lay = prob.layout
    if lay is not None and lay.T >= nsubsets:
        from ..ops.hip_host import BaselineLayout
        T, Nbase, nseg = lay.T, lay.Nbase, lay.nseg
        edges = [s * T // nsubsets for s in range(nsubsets + 1)]
        base = torch.arange(nseg, device=dev) * (T * Nbase)
        for s in order:
            t0, t1 = edges[s], edges[s + 1]
            offs = torch.arange(t0 * Nbase, t1 * Nbase, device=dev)
            sel = (base[:, None] + offs[None, :]).reshape(-1)
            sub_lay = BaselineLayout(prob.bb[sel], Nbase, t1 - t0, nseg,
                                     prob.N, dev)
            sub = LMProblem(
                prob.x[sel], prob.coh[sel], prob.bb[sel], prob.N,
                prob.nchunk,
                prob.chunk_rows[sel] if prob.chunk_rows is not None
                else None,
                prob.weights[sel] if prob.weights is not None else None,
                layout=sub_lay)
            J, _ = lm_solve(sub, J, maxiter=iters_per, **kw)
    else:
        # CPU / tiny-T path: contiguous row blocks (rows are time-major,
        # so blocks are still contiguous time ranges)
        edges = [s * B // nsubsets for s in range(nsubsets + 1)]
        for s in order:
            sel = torch.arange(edges[s], edges[s + 1], device=dev)
            sub = LMProblem(
                prob.x[sel], prob.coh[sel], prob.bb[sel], prob.N,
                prob.nchunk,
                prob.chunk_rows[sel] if prob.chunk_rows is not None
                else None,
                prob.weights[sel] if prob.weights is not None else None)
            J, _ = lm_solve(sub, J, maxiter=iters_per, **kw)
    J, info = lm_solve(prob, J, maxiter=iters_per, **kw)
    return J, info


def joint_lm_solve(x, cohs, J_packed, chunk_off, nchunks, bb, T, Nbase,
                   maxiter=10, tau=1e-3, eps1=1e-12, eps2=1e-12,
                   weights=None):
    """Joint LM over ALL clusters' parameters (cross-cluster Gauss-Newton).

    The reference polishes jointly only via LBFGS (lmfit.c:1019); a full
    joint LM converges quadratically near the solution and its JtJ/Cholesky
    are batched-GEMM shaped — cheap on MI355X. Used as the refinement stage
    after SAGE EM sweeps.

    SAGECAL_JOINT_KERNEL=1 on device tensors: the normal equations and the
    trial cost come from the kernels of joint_jtj.hip (ops.joint_jtj_jtr,
    ops.joint_cost), and with the same chunk count K > 1 in every cluster
    the K uncoupled blocks run as one batched LM (_joint_lm_blocked). With
    SAGECAL_CHOL_BLOCKED=1 as well, systems above 4096 unknowns (up to
    16384) are solved by the blocked Cholesky kernels instead of torch."""
    from ..ops import reference as R
    J = J_packed.clone()
    dev = x.device
    rdt = x.real.dtype
    Mt, N = J.shape[0], J.shape[1]
    P = 8 * Mt * N
    mu = None
    nu = 2.0
    kernels = x.is_cuda and ops.joint_kernel_on()
    if kernels:
        ncs = [int(n) for n in nchunks]
        if ncs[0] > 1 and all(n == ncs[0] for n in ncs):
            return _joint_lm_blocked(x, cohs, J, chunk_off, nchunks, bb, T,
                                     Nbase, maxiter, tau, weights)

    def assemble(Jc):
        if kernels:
            return ops.joint_jtj_jtr(x, cohs, Jc, chunk_off, nchunks, bb, T,
                                     Nbase, weights)
        return R.joint_jtj_jtr(x, cohs, Jc, chunk_off, nchunks, bb, T, Nbase,
                               weights)

    def cost_of(Jc):
        if kernels:
            return float(ops.joint_cost(x, cohs, Jc, chunk_off, nchunks, bb,
                                        T, Nbase, weights))
        V = torch.zeros_like(x)
        for ci in range(len(nchunks)):
            rows = R.chunk_rows_for(ci, nchunks, T, Nbase, x.shape[0], dev)
            if rows is None:
                rows = torch.zeros(x.shape[0], dtype=torch.long, device=dev)
            rows = rows + chunk_off[ci]
            V = V + Jc[rows, bb[:, 0]] @ cohs[ci] @ \
                Jc[rows, bb[:, 1]].conj().transpose(-1, -2)
        r = x - V
        e2 = (r.abs() ** 2).sum(dim=(-1, -2))
        if weights is not None:
            e2 = e2 * weights
        return float(e2.sum())

    H, g, cost = assemble(J)
    cost = float(cost)
    # SAGECAL_CHOL_BLOCKED=1: above the mw kernels' limit the damped solve
    # runs in the blocked Cholesky kernels, on H as it is
    hip_chol = kernels and ops.chol_blocked_on() and 4096 < P <= 16384
    if hip_chol:
        from ..ops.hip_host import chol_solve_damped
    else:
        eye = torch.eye(P, dtype=rdt, device=dev)
    for it in range(maxiter):
        if mu is None:
            mu = tau * float(H.diagonal().max())
        if float(g.abs().max()) < eps1:
            break
        failed = False
        if hip_chol:
            dp = chol_solve_damped(
                H[None], g[None],
                torch.tensor([mu], dtype=torch.float32, device=dev))[0]
            failed = bool(torch.isnan(dp).any())
        else:
            A = H + mu * eye
            try:
                L = torch.linalg.cholesky(A)
                dp = torch.cholesky_solve(g.unsqueeze(-1), L).squeeze(-1)
            except Exception:
                dp = torch.linalg.lstsq(
                    A, g.unsqueeze(-1)).solution.squeeze(-1)
        if failed:              # a NaN row: the factorisation broke down
            rho = -1.0
        else:
            Jn = J + torch.view_as_complex(
                dp.reshape(Mt, N, 2, 2, 2).contiguous())
            cn = cost_of(Jn)
            denom = float((dp * (mu * dp + g)).sum())
            rho = (cost - cn) / max(denom, 1e-300)
        if rho > 0:
            J = Jn
            cost = cn
            mu *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
            nu = 2.0
            if float(dp.norm()) < eps2 * (float(torch.view_as_real(J).norm()) + eps2):
                break
            H, g, _ = assemble(J)
        else:
            mu *= nu
            nu *= 2.0
            if nu > 1e12:
                break
    return J, cost


def _joint_lm_blocked(x, cohs, J, chunk_off, nchunks, bb, T, Nbase, maxiter,
                      tau, weights):
    """joint_lm_solve for K = nchunks[ci] > 1 chunks in every cluster on the
    blocked output of the joint kernels: chunk k of every cluster covers the
    same timeslots, so H is K uncoupled blocks of Pb = 8 M N, and they run
    as one batched LM as in _lm_solve_eager: per-block mu, gain ratio and
    accept mask, rejected blocks held with torch.where, no host reads inside
    the loop. Blocks are independent problems; against the scalar loop only
    the damping differs, one mu per block instead of one for all."""
    from ..ops.hip_host import chol_solve_damped
    M, K = len(nchunks), int(nchunks[0])
    N = J.shape[1]
    Pb = 8 * M * N
    args = (chunk_off, nchunks, bb, T, Nbase, weights)

    def step_to_jones(dp):
        # block k, order (cluster, station, 8) -> chunk ci*K + k of J
        d = dp.reshape(K, M, N, 2, 2, 2).transpose(0, 1)
        return torch.view_as_complex(d.reshape(M * K, N, 2, 2, 2).contiguous())

    def per_chunk(v):                       # [K] -> [M*K, 1, 1, 1]
        return v.repeat(M)[:, None, None, None]

    H, g, cost = ops.joint_jtj_jtr(x, cohs, J, *args, blocked=True)
    mu = tau * H.diagonal(dim1=-2, dim2=-1).max(dim=-1).values
    nu = torch.full_like(mu, 2.0)
    for it in range(maxiter):
        # the Cholesky kernels' limit: 4096, or with SAGECAL_CHOL_BLOCKED=1
        # the 16384 of the blocked kernels
        if Pb <= 4096 or (ops.chol_blocked_on() and Pb <= 16384):
            dp = chol_solve_damped(H, g, mu)
        else:
            # H is rebuilt before its next use. One block at a time, the
            # single-matrix solver the scalar loop uses: torch's batched
            # Cholesky of [16, 5120, 5120] ended in a launch failure on
            # the MI355X
            H.diagonal(dim1=-2, dim2=-1).add_(mu[:, None])
            dp = torch.stack([_chol_solve(H[k], g[k]) for k in range(K)])
        dp = torch.nan_to_num(dp, nan=0.0, posinf=0.0, neginf=0.0)
        Jn = J + step_to_jones(dp)
        cn = ops.joint_cost(x, cohs, Jn, *args, blocked=True)
        denom = (dp * (mu[:, None] * dp + g)).sum(dim=-1).clamp_min(1e-30)
        rho = (cost - cn) / denom
        accept = rho > 0
        J = torch.where(per_chunk(accept), Jn, J)
        cost = torch.where(accept, cn, cost)
        fac = (1.0 - (2.0 * rho - 1.0) ** 3).clamp_min(1.0 / 3.0)
        mu = torch.where(accept, mu * fac, mu * nu)
        nu = torch.where(accept, torch.full_like(nu, 2.0), nu * 2.0)
        if it + 1 < maxiter:
            H, g, _ = ops.joint_jtj_jtr(x, cohs, J, *args, blocked=True)
    return J, float(cost.sum())


def _lm_body(x, coh, bb, N, nchunk, chunk_rows, weights, layout, J0,
             maxiter, tau, prob):
    """The capture-safe fixed-iteration LM loop (no host reads)."""
    dev = x.device
    rdt = x.real.dtype
    from ..ops.hip_host import chol_solve_damped
    J = J0.clone()
    nu = torch.full((nchunk,), 2.0, dtype=rdt, device=dev)

    def full_cost(Jc):
        c = ops.model_cost_per_chunk(x, coh, Jc, bb, N, weights, chunk_rows,
                                     nchunk, layout)
        if prob.admm is not None:
            c = c + _admm_cost(Jc, prob).to(c.dtype)
        return c

    JtJ, Jtr, _ = ops.jtj_jtr(x, coh, J, bb, N, weights, chunk_rows,
                              nchunk, layout)
    JtJ, Jtr = _apply_admm_terms(JtJ, Jtr, J, prob, N, nchunk)
    cost = full_cost(J)
    init_cost = cost.clone()
    diag_max = JtJ.diagonal(dim1=-2, dim2=-1).max(dim=-1).values
    mu = tau * diag_max
    for it in range(maxiter):
        dp = chol_solve_damped(JtJ, Jtr, mu)
        dp = torch.nan_to_num(dp, nan=0.0, posinf=0.0, neginf=0.0)
        Jnew = J + _vec_to_jones(dp, nchunk, N)
        cost_new = full_cost(Jnew)
        denom = (dp * (mu[:, None] * dp + Jtr)).sum(dim=-1).clamp_min(1e-30)
        rho = (cost - cost_new) / denom
        accept = rho > 0
        J = torch.where(accept[:, None, None, None], Jnew, J)
        cost = torch.where(accept, cost_new, cost)
        fac = (1.0 - (2.0 * rho - 1.0) ** 3).clamp_min(1.0 / 3.0)
        mu = torch.where(accept, mu * fac, mu * nu)
        nu = torch.where(accept, torch.full_like(nu, 2.0), nu * 2.0)
        if it + 1 < maxiter:
            JtJ, Jtr, _ = ops.jtj_jtr(x, coh, J, bb, N, weights, chunk_rows,
                                      nchunk, layout)
            JtJ, Jtr = _apply_admm_terms(JtJ, Jtr, J, prob, N, nchunk)
    return J, cost, init_cost


def _lm_solve_graphed(prob, J0, maxiter, tau, eps1, eps2):
    """hipGraph-captured LM: one replay per solve, zero per-iteration host
    dispatch. Static input buffers per (B, nchunk, maxiter, layout) shape."""
    x, coh, bb, N = prob.x, prob.coh, prob.bb, prob.N
    nchunk = prob.nchunk
    dev = x.device
    B = x.shape[0]
    key = (B, nchunk, N, maxiter, ops.obj_token(prob.layout), float(tau),
           prob.admm is not None)
    ent = _lm_graph_cache.get(key)
    if ent is None:
        ent = {}
        ent['x'] = torch.empty_like(x)
        ent['coh'] = torch.empty_like(coh)
        ent['J0'] = torch.empty_like(J0)
        ent['w'] = torch.ones(B, dtype=torch.float32, device=dev)
        ent['rows'] = torch.zeros(B, dtype=torch.long, device=dev)
        ent['bb'] = bb

        class _P:  # static stand-in problem carrying the admm statics
            pass
        sp = _P()
        sp.admm = None
        if prob.admm is not None:
            rho_a, Y_a, BZ_a = prob.admm
            ent['admm'] = (torch.empty_like(rho_a), torch.empty_like(Y_a),
                           torch.empty_like(BZ_a))
            sp.admm = ent['admm']
        ent['sp'] = sp
        # warmup on a side stream (allocator + kernels)
        ent['x'].copy_(x); ent['coh'].copy_(coh); ent['J0'].copy_(J0)
        if prob.weights is not None:
            ent['w'].copy_(prob.weights.to(torch.float32))
        if prob.chunk_rows is not None:
            ent['rows'].copy_(prob.chunk_rows)
        if prob.admm is not None:
            for d, sr in zip(ent['admm'], prob.admm):
                d.copy_(sr)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(2):
                _lm_body(ent['x'], ent['coh'], ent['bb'], N, nchunk,
                         ent['rows'], ent['w'], prob.layout, ent['J0'],
                         maxiter, tau, sp)
        torch.cuda.current_stream().wait_stream(st)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = _lm_body(ent['x'], ent['coh'], ent['bb'], N, nchunk,
                            ent['rows'], ent['w'], prob.layout, ent['J0'],
                            maxiter, tau, sp)
        ent['graph'] = g
        ent['outs'] = outs
        _lm_graph_cache[key] = ent
    ent['x'].copy_(x)
    ent['coh'].copy_(coh)
    ent['J0'].copy_(J0)
    if prob.weights is not None:
        ent['w'].copy_(prob.weights.to(torch.float32))
    else:
        ent['w'].fill_(1.0)
    if prob.chunk_rows is not None:
        ent['rows'].copy_(prob.chunk_rows)
    else:
        ent['rows'].zero_()
    if prob.admm is not None:
        for d, sr in zip(ent['admm'], prob.admm):
            d.copy_(sr)
    ent['graph'].replay()
    J, cost, init_cost = ent['outs']
    return J.clone(), {'init_cost': init_cost.clone(),
                       'final_cost': cost.clone(), 'niter': maxiter}


_robust_graph_cache = {}


def _robust_body(x, coh, bb, N, nchunk, chunk_rows, layout, J0, nu_t,
                 inner, tau, prob_admm):
    """Capture-safe robust IRLS body (robust_outer=1 schedule):
    solve -> Student's-t weight update (stale nu, refreshed on the host
    after replay) -> weighted solve. Returns (J, w, e2sum)."""
    class _P:
        pass
    p1 = _P(); p1.admm = prob_admm
    J1, _, init_cost = _lm_body(x, coh, bb, N, nchunk, chunk_rows, None,
                                layout, J0, inner, tau, p1)
    from ..ops import dispatch as ops_d
    V = ops_d.apply_jones(coh, J1, bb, chunk_rows, layout)
    r = x - V
    e2 = (r.abs() ** 2).sum(dim=(-1, -2)).to(torch.float32)
    w = (nu_t + 8.0) / (nu_t + e2)
    J2, cost, _ = _lm_body(x, coh, bb, N, nchunk, chunk_rows, w, layout,
                           J1, inner, tau, p1)
    logsumw = (torch.log(w) - w).mean()
    return J2, w, cost, init_cost, logsumw


def robust_lm_graphed(prob, J0, nu0, inner, tau=1e-3):
    """hipGraph-captured robust LM (one replay for the whole IRLS
    schedule). The nu AECM update runs on the host AFTER the replay from
    the captured mean(log w - w) (one sync per group-solve)."""
    x, coh, bb, N = prob.x, prob.coh, prob.bb, prob.N
    nchunk = prob.nchunk
    dev = x.device
    B = x.shape[0]
    key = ('robust', B, nchunk, N, inner, ops.obj_token(prob.layout),
           prob.admm is not None)
    ent = _robust_graph_cache.get(key)
    if ent is None:
        ent = {'x': torch.empty_like(x), 'coh': torch.empty_like(coh),
               'J0': torch.empty_like(J0),
               'rows': torch.zeros(B, dtype=torch.long, device=dev),
               'nu': torch.zeros((), dtype=torch.float32, device=dev),
               'bb': bb}
        ent['admm'] = None
        if prob.admm is not None:
            ent['admm'] = tuple(torch.empty_like(t) for t in prob.admm)
        ent['x'].copy_(x); ent['coh'].copy_(coh); ent['J0'].copy_(J0)
        if prob.chunk_rows is not None:
            ent['rows'].copy_(prob.chunk_rows)
        ent['nu'].fill_(nu0)
        if prob.admm is not None:
            for d, sr in zip(ent['admm'], prob.admm):
                d.copy_(sr)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(2):
                _robust_body(ent['x'], ent['coh'], ent['bb'], N, nchunk,
                             ent['rows'], prob.layout, ent['J0'],
                             ent['nu'], inner, tau, ent['admm'])
        torch.cuda.current_stream().wait_stream(st)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = _robust_body(ent['x'], ent['coh'], ent['bb'], N, nchunk,
                                ent['rows'], prob.layout, ent['J0'],
                                ent['nu'], inner, tau, ent['admm'])
        ent['graph'] = g
        ent['outs'] = outs
        _robust_graph_cache[key] = ent
    ent['x'].copy_(x)
    ent['coh'].copy_(coh)
    ent['J0'].copy_(J0)
    if prob.chunk_rows is not None:
        ent['rows'].copy_(prob.chunk_rows)
    else:
        ent['rows'].zero_()
    ent['nu'].fill_(nu0)
    if prob.admm is not None:
        for d, sr in zip(ent['admm'], prob.admm):
            d.copy_(sr)
    ent['graph'].replay()
    J, w, cost, init_cost, logsumw = ent['outs']
    return (J.clone(), float(logsumw),
            {'init_cost': init_cost.clone(), 'final_cost': cost.clone()})
