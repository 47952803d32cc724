"""Op dispatch: CUDA tensors -> the HIP/CDNA4 extension, CPU -> the PyTorch
reference implementation.

The HIP extension is MANDATORY on GPU: if a CUDA tensor reaches an op and
the extension is missing, we raise (no silent eager fallback — the driver's
round-end check verifies the native .so is actually loaded).
Set SAGECAL_FORCE_REFERENCE=1 to explicitly run the torch reference on GPU
(used only for kernel A/B numerics tests).
"""
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
                         Nbase=0):
    """Coherencies of every channel of `freqs`, [F, M, R, 2, 2], or with
    reduce='mean' their mean over the channels [M, R, 2, 2]; fdelta is the
    width of one channel. Optional station beam per channel: `beam`
    [F, T, K, N] gains and/or `ejones` [F, T, K, NE, 2, 2] (or
    [F, T, K, 2, 2]) patterns, with `pairs` [Nbase, 2]. On the GPU one launch
    of the all-channels kernel (no shapelet sources: ValueError); elsewhere
    the per-channel loop over the fp64 reference, with a beam over
    beams.predict_coh_withbeam."""
    if _use_hip(u):
        from . import hip_host
        return hip_host.predict_coh_channels(
            pack, u, v, w, freqs, freq0, fdelta, tdelta, dec0, reduce,
            beam=beam, ejones=ejones, pairs=pairs, Nbase=Nbase)
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
                        ejones=None):
    """x[f] - sum over clusters with subtract[ci] of J_p C_f J_q^H,
    [F, R, 2, 2], C_f with the station beam of `beam` [F, T, K, N] and/or
    `ejones` [F, T, K, NE, 2, 2] (or [F, T, K, 2, 2]) when given. J [Mt, N, 2, 2] packed solutions; chunk_tab [M, T] global
    chunk id per (cluster, timeslot); pairs [Nbase, 2], rows r = t*Nbase + b;
    a row whose pair has a negative entry keeps x. On the GPU one launch of
    the fused kernel (no shapelet sources: ValueError); elsewhere the
    per-channel loop over R.predict_coh (with a beam,
    beams.predict_coh_withbeam) and R.apply_jones."""
    if _use_hip(u):
        from . import hip_host
        return hip_host.residuals_multifreq(
            pack, x, u, v, w, freqs, freq0, fdelta, tdelta, dec0, J,
            chunk_tab, pairs, subtract, beam=beam, ejones=ejones)
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


def lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks, bb, T, Nbase,
                    robust_nu=None, weights=None):
    if _use_hip(x):
        from . import hip_host
        return hip_host.lbfgs_cost_grad(x, cohs, J_packed, chunk_off,
                                        nchunks, bb, T, Nbase, robust_nu,
                                        weights)
    return R.lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks, bb, T,
                             Nbase, robust_nu, weights)
