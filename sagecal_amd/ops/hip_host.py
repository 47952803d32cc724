"""Host-side adapters between the dispatch API and the gfx950 kernels.

Handles layout preparation: per-frequency flux scaling (done with torch on
device, keeping the predict kernel free of spectral-index math), baking the
projection identity into unused rotation terms, the device-resident
shapelet mode table, chunk tables, station-pair index tables, and
complex64 views.
"""
import math
import os

import torch

from . import dispatch

_pidx_cache = {}     # (N, Nbase, device) -> (host table, device table)
_layout_memo = {}    # (bb token, version, Nbase, N, device) -> (pairs, pidx)


def _ext():
    e = dispatch._load_ext()
    if e is None:
        raise RuntimeError(
            f"dirac_hip extension unavailable: {dispatch._ext_err}")
    return e


class ShapeletTable:
    """Device-resident table of the pack's shapelet sources, read by
    k_shapelet_coh and by shapelet_coh_torch. Built once from the host-side
    `pack.shapelets` dict; S entries sorted by global source index, so
    cluster ids are non-decreasing.

      src, cluster, n0   int32 [S]    global source / cluster index, order
      beta               float [S]    shapelet scale
      off                int32 [S+1]  prefix sum of n0^2
      coef               float [off[S]]  mode (n1,n2) of entry s at
                         off[s] + n2*n0 + n1, holding
                         modes[n2*n0+n1] * sgn(n1+n2) * 2 pi a b with
                         sgn(k) = +1 for k mod 4 in {0,1}, else -1: the
                         mode value is i^(n1+n2) phi_n1 phi_n2, so the
                         parity of n1+n2 alone picks the real or the
                         imaginary accumulator
      cxi,sxi,cphi,sphi  float [S]    projection rotation, identity
                         (1,0,1,0) when the source's use_proj is off
      psign              float [S]    -1 with use_proj (the shapelet
                         projection is the NEGATED gaussian one,
                         shapelet.shapelet_contrib), else +1
      a, b, ceP, seP     float [S]    1/eX, 1/eY, cos(eP), sin(eP)
      ll, mm, nn1        float64 [S]  direction cosines
      rec                float [2, max n0]  recurrence constants
                         sqrt(2/n), sqrt((n-1)/n); rec[:,0] unused

    `float` is float32, the kernel's layout; dtype=torch.float64 keeps the
    host-computed values unrounded for fp64 checks of the mirror. The
    main-kernel rotation arrays of GPUPack bake use_proj | stype>=2, which
    is wrong for shapelets, so the table bakes its own."""

    FIELDS = ('src', 'cluster', 'n0', 'beta', 'off', 'coef', 'cxi', 'sxi',
              'cphi', 'sphi', 'psign', 'a', 'b', 'ceP', 'seP', 'll', 'mm',
              'nn1', 'rec')

    def __init__(self, pack, device, dtype=torch.float32):
        import numpy as np
        items = sorted(pack.shapelets.items())
        src = np.array([g for g, _ in items], dtype=np.int64)
        host = lambda t: t.detach().cpu().to(torch.float64).numpy()[src]
        co = pack.cluster_off.detach().cpu().numpy()
        n0 = np.array([sh[0] for _, sh in items], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(n0 * n0)])
        proj = pack.use_proj.detach().cpu().numpy()[src] != 0
        a, b = 1.0 / host(pack.eX), 1.0 / host(pack.eY)
        eP = host(pack.eP)
        coef = np.zeros(int(off[-1]))
        for s, (_, (n, _beta, modes)) in enumerate(items):
            k = np.arange(n)
            nsum = k[None, :] + k[:, None]               # [n2, n1]
            sgn = np.where(nsum % 4 < 2, 1.0, -1.0)
            m = np.asarray(modes, dtype=np.float64).reshape(n, n)
            coef[off[s]:off[s + 1]] = (
                m * sgn * (2.0 * math.pi * a[s] * b[s])).reshape(-1)
        self.nmax = int(n0.max())
        rec = np.zeros((2, self.nmax))
        k = np.arange(1, self.nmax)
        rec[0, 1:] = np.sqrt(2.0 / k)
        rec[1, 1:] = np.sqrt((k - 1.0) / k)
        # dense [S, n2, n1] view of coef for the torch mirror: index into
        # coef, or one past its end (a zero slot) beyond the entry's order
        k = np.arange(self.nmax)
        idx = off[:-1, None, None] + k[None, :, None] * n0[:, None, None] \
            + k[None, None, :]
        inside = (k[None, :, None] < n0[:, None, None]) & \
            (k[None, None, :] < n0[:, None, None])
        self.S = len(items)
        self.M = int(pack.M)
        self.K = int(pack.K) if hasattr(pack, 'K') else int(co[-1])
        i32 = lambda x: torch.as_tensor(
            np.ascontiguousarray(x), dtype=torch.int32).to(device)
        flt = lambda x, dt=dtype: torch.as_tensor(
            np.ascontiguousarray(x), dtype=torch.float64).to(
                device=device, dtype=dt).contiguous()
        self.src = i32(src)
        self.cluster = i32(np.searchsorted(co, src, side='right') - 1)
        self.n0 = i32(n0)
        self.off = i32(off)
        self.beta = flt([sh[1] for _, sh in items])
        self.coef = flt(coef)
        self.cxi = flt(np.where(proj, host(pack.cxi), 1.0))
        self.sxi = flt(np.where(proj, host(pack.sxi), 0.0))
        self.cphi = flt(np.where(proj, host(pack.cphi), 1.0))
        self.sphi = flt(np.where(proj, host(pack.sphi), 0.0))
        self.psign = flt(np.where(proj, -1.0, 1.0))
        self.a, self.b = flt(a), flt(b)
        self.ceP, self.seP = flt(np.cos(eP)), flt(np.sin(eP))
        self.ll = flt(host(pack.ll), torch.float64)
        self.mm = flt(host(pack.mm), torch.float64)
        self.nn1 = flt(host(pack.nn1), torch.float64)
        self.rec = flt(rec)
        self.cluster_long = self.cluster.long()
        self.src_long = self.src.long()
        self.pad_idx = torch.as_tensor(
            np.where(inside, idx, int(off[-1]))).to(device)


def shapelet_coh_torch(tab, flux, r1, u, v, w, freq, fdelta, tdelta,
                       beam=None, pairs=None, Nbase=0):
    """Vectorised torch mirror of k_shapelet_coh over [B, S]: coherencies
    [M, B, 2, 2] of the table's shapelet sources only, on the device and in
    the real dtype of `u`, with no host synchronisation. flux: [4, S]
    I,Q,U,V at the channel; r1: [S] time-smear distance term; optional
    beam [T, K, N] and pairs [Nbase, 2] as in predict_coh."""
    rt = u.dtype
    c = lambda t: t.to(rt)
    uc, vc, wc = u[:, None], v[:, None], w[:, None]
    two_pi = 2.0 * math.pi
    G = two_pi * (uc * c(tab.ll) + vc * c(tab.mm) + wc * c(tab.nn1))
    ph = torch.fmod(G * freq, two_pi)
    smf = G * (fdelta * 0.5)
    big = smf.abs() > 1e-9
    sm = torch.where(big, (torch.sin(smf)
                           / torch.where(big, smf, torch.ones_like(smf))
                           ).abs(), torch.ones_like(smf))
    blf = torch.sqrt(uc * uc + vc * vc + wc * wc) * freq
    prod = (7.2921150e-5 * float(tdelta)) * blf * c(r1)
    sm = sm * torch.where(prod > 1e-9, 1.0645 * torch.erf(0.8326 * prod)
                          / prod.clamp_min(1e-9), torch.ones_like(prod))
    phc = torch.complex(torch.cos(ph) * sm, torch.sin(ph) * sm)
    uf, vf, wf = uc * freq, vc * freq, wc * freq
    cxi, sxi = c(tab.cxi), c(tab.sxi)
    cphi, sphi = c(tab.cphi), c(tab.sphi)
    up = c(tab.psign) * (uf * cxi - vf * cphi * sxi + wf * sphi * sxi)
    vp = c(tab.psign) * (uf * sxi + vf * cphi * cxi - wf * sphi * cxi)
    ut = c(tab.a) * (c(tab.ceP) * up - c(tab.seP) * vp)
    vt = c(tab.b) * (c(tab.seP) * up + c(tab.ceP) * vp)
    beta = c(tab.beta)
    rec = c(tab.rec)

    def phi(x):                       # [B, S] -> [B, S, nmax]
        cols = [math.sqrt(0.5) * torch.exp(-0.5 * x * x)]
        prev = torch.zeros_like(x)
        for n in range(1, tab.nmax):
            cols.append(x * rec[0, n] * cols[-1] - rec[1, n] * prev)
            prev = cols[-2]
        return torch.stack(cols, dim=-1)
    pu, pv = phi(-ut * beta), phi(vt * beta)
    coef = torch.cat([c(tab.coef), torch.zeros(1, dtype=rt,
                                               device=u.device)])
    cd = coef[tab.pad_idx]                                   # [S, n2, n1]
    k = torch.arange(tab.nmax, device=u.device)
    odd = ((k[:, None] + k[None, :]) % 2 == 1).to(rt)
    re = torch.einsum('bsk,skl,bsl->bs', pv, cd * (1.0 - odd), pu)
    im = torch.einsum('bsk,skl,bsl->bs', pv, cd * odd, pu)
    term = phc * torch.complex(re, im)
    if beam is not None:
        B = u.shape[0]
        Nbase = int(Nbase) or int(pairs.shape[0])
        row = torch.arange(B, device=u.device)
        t, bl = row // Nbase, row % Nbase
        p, q = pairs[bl, 0].long(), pairs[bl, 1].long()
        g = tab.src_long[None, :]
        term = term * c(beam[t[:, None], g, p[:, None]]
                        * beam[t[:, None], g, q[:, None]])
    fI, fQ, fU, fV = (term * c(flux[i]) for i in range(4))
    coh = torch.stack([fI + fQ, fU + 1j * fV, fU - 1j * fV, fI - fQ],
                      dim=-1)                                # [B, S, 4]
    out = torch.zeros(tab.M, u.shape[0], 4, dtype=coh.dtype,
                      device=u.device)
    out.index_add_(0, tab.cluster_long, coh.permute(1, 0, 2).contiguous())
    return out.view(tab.M, -1, 2, 2)


class GPUPack:
    """Device-resident SourcePack in kernel layout (float32 props, float64
    direction cosines, projection identity baked for use_proj=False)."""

    def __init__(self, pack, device):
        f32 = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        f64 = lambda t: t.to(device=device, dtype=torch.float64).contiguous()
        self.M = pack.M
        self.K = int(pack.cluster_off[-1])       # sources in the pack
        self.ll, self.mm, self.nn1 = f64(pack.ll), f64(pack.mm), f64(pack.nn1)
        for k in ('sI', 'sQ', 'sU', 'sV', 'sI0', 'sQ0', 'sU0', 'sV0',
                  'spec_idx', 'spec_idx1', 'spec_idx2', 'eX', 'eY', 'eP'):
            setattr(self, k, f32(getattr(pack, k)))
        self.f0 = pack.f0.to(device=device, dtype=torch.float64)
        # gaussian honors use_projection; disk/ring ALWAYS project
        # (disk_contrib/ring_contrib predict.c:60-90, oracle-verified)
        up = pack.use_proj.to(device=device).bool() | \
            (pack.stype.to(device) >= 2)
        one = torch.ones_like(f32(pack.cxi))
        zero = torch.zeros_like(one)
        self.cxi = torch.where(up, f32(pack.cxi), one).contiguous()
        self.sxi = torch.where(up, f32(pack.sxi), zero).contiguous()
        self.cphi = torch.where(up, f32(pack.cphi), one).contiguous()
        self.sphi = torch.where(up, f32(pack.sphi), zero).contiguous()
        self.stype = pack.stype.to(device=device,
                                   dtype=torch.int32).contiguous()
        # shapelet sources go through k_shapelet_coh from the table below:
        # zero their fluxes in the main-kernel arrays so they contribute
        # nothing there, and keep the true ones gathered per table entry
        self.sh = None
        if getattr(pack, 'shapelets', None):
            self.sh = ShapeletTable(pack, device)
            src = self.sh.src
            gather = lambda ks: torch.stack(
                [getattr(self, k).index_select(0, src) for k in ks]
            ).contiguous()
            self._sh_flux = gather(('sI', 'sQ', 'sU', 'sV'))        # [4,S]
            self._sh_flux0 = gather(('sI0', 'sQ0', 'sU0', 'sV0'))
            sh = self.stype == 4
            for k in ('sI', 'sQ', 'sU', 'sV', 'sI0', 'sQ0', 'sU0', 'sV0'):
                t = getattr(self, k).clone()
                t[sh] = 0.0
                setattr(self, k, t.contiguous())
        self.pack_ref = pack
        # zero shape angles for point sources keep the envelope branch out
        self.cluster_off = pack.cluster_off.to(device=device,
                                               dtype=torch.int32).contiguous()
        self.freq0 = None
        self._flux_cache = {}
        self._sh_flux_cache = {}
        self._stack_cache = {}

    def _flog(self, freq):
        """Log-polynomial spectral exponent per source at `freq`."""
        lf = torch.log(torch.tensor(float(freq), dtype=torch.float64,
                                    device=self.ll.device) / self.f0)
        lf = lf.to(torch.float32)
        return (self.spec_idx * lf + self.spec_idx1 * lf ** 2
                + self.spec_idx2 * lf ** 3)

    @staticmethod
    def _scale(s0, flog):
        mag = torch.exp(torch.log(s0.abs().clamp_min(1e-30)) + flog)
        return torch.where(s0 == 0, torch.zeros_like(s0),
                           torch.sign(s0) * mag)

    def fluxes_at(self, freq, freq0):
        """Per-source fluxes at channel `freq`; pack fluxes are given at
        freq0 (sI..) and catalogue f0 (sI0..). Shapelet sources are zero
        here; their fluxes at the same channel are cached alongside
        (shapelet_fluxes_at)."""
        key = round(float(freq), 3)
        if key in self._flux_cache:
            return self._flux_cache[key]
        if abs(freq - freq0) < 1.0:
            out = (self.sI, self.sQ, self.sU, self.sV)
            if self.sh is not None:
                self._sh_flux_cache[key] = self._sh_flux
        else:
            flog = self._flog(freq)
            out = tuple(self._scale(s0, flog) for s0 in
                        (self.sI0, self.sQ0, self.sU0, self.sV0))
            if self.sh is not None:
                self._sh_flux_cache[key] = self._scale(
                    self._sh_flux0,
                    flog.index_select(0, self.sh.src)).contiguous()
        self._flux_cache[key] = out
        return out

    def flux_stack(self, freqs, freq0):
        """(fluxes [F, 4, K] float32, freqs [F] float64) on the device for
        the all-channels kernels: row f stacks fluxes_at(freqs[f], freq0),
        so a channel within 1 Hz of freq0 carries the pack fluxes and every
        other one the spectral-index scaling of the catalogue fluxes.
        Remembered per frequency tuple."""
        key = (tuple(round(float(f), 3) for f in freqs),
               round(float(freq0), 3))
        hit = self._stack_cache.get(key)
        if hit is None:
            if len(self._stack_cache) > 16:   # bound long multi-MS runs
                self._stack_cache.pop(next(iter(self._stack_cache)))
            flux = torch.stack([torch.stack(self.fluxes_at(float(f), freq0))
                                for f in freqs]).contiguous()
            fq = torch.tensor([float(f) for f in freqs], dtype=torch.float64,
                              device=self.ll.device)
            hit = self._stack_cache[key] = (flux, fq)
        return hit

    def shapelet_fluxes_at(self, freq, freq0):
        """Un-zeroed I, Q, U, V of the shapelet sources at channel `freq`,
        [4, S] float32 in table order."""
        self.fluxes_at(freq, freq0)
        return self._sh_flux_cache[round(float(freq), 3)]

    def r1_for(self, dec0):
        """Time-smear source-distance term sqrt(ll^2+(sin(dec0) mm)^2)
        (predict.c:98-100), per source."""
        ds = math.sin(dec0)
        return torch.sqrt(self.ll ** 2 + (ds * self.mm) ** 2).to(
            torch.float32).contiguous()


_gpu_pack_cache = {}


def gpu_pack(pack, device):
    key = (dispatch.obj_token(pack), str(device))
    if key not in _gpu_pack_cache:
        if len(_gpu_pack_cache) > 16:   # bound long multi-MS runs
            _gpu_pack_cache.pop(next(iter(_gpu_pack_cache)))
        _gpu_pack_cache[key] = GPUPack(pack, device)
    return _gpu_pack_cache[key]


_nsta_memo = {}      # (table token, version) -> (min, max) entry


def _pair_range(pairs):
    """(min, max) entry of a device index table (station pairs, chunk
    ids). Reads it back to the host, so the answer is remembered per
    tensor."""
    try:
        key = (dispatch.obj_token(pairs), pairs._version)
    except RuntimeError:                 # inference tensor: no version
        key = None
    hit = _nsta_memo.get(key)
    if hit is None:
        hit = (int(pairs.min()), int(pairs.max()))
        if key is not None:
            if len(_nsta_memo) > 64:
                _nsta_memo.pop(next(iter(_nsta_memo)))
            _nsta_memo[key] = hit
    return hit


def _check_ejones(ejones, beam, pairs, Nbase, R, K):
    """Host-side contract of the E-Jones kernels, which index ejones and
    beam by timeslot, source and station with no checks of their own.
    Returns the station count N."""
    if pairs is None:
        raise ValueError("ejones needs the station-pair table `pairs`")
    if ejones.dim() != 5 or tuple(ejones.shape[3:]) != (2, 2):
        raise ValueError("ejones must be [T, K, NE, 2, 2], got "
                         f"{tuple(ejones.shape)}")
    Nbase = int(Nbase) or int(pairs.shape[0])
    if pairs.dim() != 2 or pairs.shape[0] < Nbase or pairs.shape[1] != 2:
        raise ValueError("pairs must be [Nbase, 2]")
    T, Ke, NE = (int(x) for x in ejones.shape[:3])
    if T * Nbase != R:
        raise ValueError(f"ejones has {T} timeslots of {Nbase} baselines, "
                         f"the predict has {R} rows")
    if Ke < K:
        raise ValueError(f"ejones covers {Ke} sources, the pack has {K}")
    lo, hi = _pair_range(pairs)
    if beam is not None:
        if tuple(beam.shape[:2]) != (T, Ke):
            raise ValueError("beam and ejones disagree on [T, K]")
        N = int(beam.shape[2])
    else:
        N = NE if NE != 1 else hi + 1
    if lo < 0 or hi >= N:
        raise ValueError(f"pairs name stations {lo}..{hi}, outside the "
                         f"{N} stations of the beam buffers")
    if NE not in (1, N):
        raise ValueError(f"ejones holds {NE} patterns per source; must be "
                         f"1 or the station count {N}")
    return N


def predict_coh(pack, u, v, w, freq, freq0, fdelta, tdelta, dec0,
                beam=None, pairs=None, Nbase=0, ejones=None, **kw):
    """Kernel-backed coherency predict. Optional fused station beam
    (-B 1, reference DOBEAM_ARRAY): `beam` [T, K, N] float32 real
    array-factor gains on device + `pairs` [Nbase, 2] int32 — each
    source's contribution is scaled by beam[t,k,p]*beam[t,k,q] inside
    k_predict_coh (predict_model.cu:843-852 semantics). Shapelet sources
    (gp.sh) are added by k_shapelet_coh on the same stream, beam-scaled
    the same way; once the pack is on the device this path has no host
    synchronisation. SAGECAL_SHAPELET_HOST=1 swaps that kernel for its
    torch mirror shapelet_coh_torch.

    Optional element beam (-B 2/3, DOBEAM_FULL / DOBEAM_ELEMENT): `ejones`
    [T, K, NE, 2, 2] complex64, NE = 1 (one dipole pattern per array
    origin) or N (one per station). Each source then contributes
    g_p g_q E_p C E_q^H with E_s = ejones[t, k, s if NE == N else 0] and
    g = beam[t,k,.] (1 without `beam`), through the _ej variants of both
    kernels. `pairs` is required with it. The first call with a new pair
    table reads its index range back for the bounds check."""
    gp = pack if isinstance(pack, GPUPack) else gpu_pack(pack, u.device)
    sI, sQ, sU, sV = gp.fluxes_at(freq, freq0)
    r1 = gp.r1_for(dec0)
    u64 = u.to(torch.float64).contiguous()
    v64 = v.to(torch.float64).contiguous()
    w64 = w.to(torch.float64).contiguous()
    Nsta = 0
    if ejones is not None:
        if os.environ.get('SAGECAL_SHAPELET_HOST') == '1' \
                and gp.sh is not None:
            raise RuntimeError("the torch shapelet mirror has no E-Jones")
        Nsta = _check_ejones(ejones, beam, pairs, Nbase, int(u.shape[0]),
                             gp.K)
        ejones = ejones.to(device=u.device,
                           dtype=torch.complex64).contiguous()
    if beam is not None or ejones is not None:
        if beam is not None:
            beam = beam.to(device=u.device,
                           dtype=torch.float32).contiguous()
        Nbase = int(Nbase) or int(pairs.shape[0])
        pairs = pairs[:Nbase].to(device=u.device,
                                 dtype=torch.int32).contiguous()
    ej = {} if ejones is None else {'ejones': ejones, 'Nsta': Nsta}
    out = _ext().predict_coh(
        u64, v64, w64, gp.ll, gp.mm, gp.nn1, sI, sQ, sU, sV,
        gp.eX, gp.eY, gp.eP, gp.cxi, gp.sxi, gp.cphi, gp.sphi, r1,
        gp.stype, gp.cluster_off, float(freq), float(fdelta) * 0.5,
        float(tdelta), beam=beam, pairs=pairs, Nbase=int(Nbase), **ej)
    if gp.sh is not None:
        tab = gp.sh
        flux = gp.shapelet_fluxes_at(freq, freq0)
        r1s = r1.index_select(0, tab.src)
        if beam is not None and beam.shape[1] < tab.K:
            raise ValueError("beam covers fewer sources than the pack")
        if os.environ.get('SAGECAL_SHAPELET_HOST') == '1':
            # torch mirror of the kernel (same table), for cross-checks
            add = shapelet_coh_torch(tab, flux, r1s, u64, v64, w64,
                                     float(freq), float(fdelta),
                                     float(tdelta), beam, pairs, Nbase)
            out = out + add.reshape(gp.M, -1, 4).to(out.dtype)
        else:
            _ext().shapelet_coh_add(
                out, u64, v64, w64, *(getattr(tab, k) for k in tab.FIELDS),
                flux, r1s, float(freq), float(fdelta) * 0.5, float(tdelta),
                beam=beam, pairs=pairs, Nbase=int(Nbase), **ej)
    return out.view(gp.M, -1, 2, 2)


def _mf_source_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0):
    """Positional arguments u .. tdelta of the extension's all-channels
    entry points."""
    flux, fq = gp.flux_stack(freqs, freq0)
    f64 = lambda t: t.to(torch.float64).contiguous()
    return (f64(u), f64(v), f64(w), gp.ll, gp.mm, gp.nn1, flux, gp.eX,
            gp.eY, gp.eP, gp.cxi, gp.sxi, gp.cphi, gp.sphi, gp.r1_for(dec0),
            gp.stype, gp.cluster_off, fq, float(fdelta) * 0.5, float(tdelta))


def _mf_pack(pack, device, what):
    gp = pack if isinstance(pack, GPUPack) else gpu_pack(pack, device)
    if gp.sh is not None:
        raise ValueError(f"{what} has no shapelet sources; predict this "
                         "pack channel by channel with predict_coh")
    return gp


def _check_beam_channels(beam, ejones, pairs, Nbase, F, R, K, dev,
                         negative_ok=False, Nsta=None):
    """Host-side contract of the beamed all-channels kernels, which index
    beam [F, T, Ke, N] and ejones [F, T, Ke, NE, 2, 2] (or [F, T, Ke, 2, 2],
    one pattern, NE = 1) by channel, timeslot, source and station with no
    checks of their own. Checked once here, as _check_ejones does for one
    channel: leading dimension F, [T, Ke] agreement, Ke >= K, the station
    range of `pairs` inside N, NE in (1, N). negative_ok: the residual
    kernels keep x on a row with a negative pair entry and look nothing up
    for it, the predict kernels have no such row. Nsta: the station count
    when the caller has one (J's), else beam's, else NE or the largest pair
    entry + 1. Returns the keyword arguments of the extension: beam
    float32, ejones complex64 six-dimensional, pairs int32 [Nbase, 2], all
    contiguous on `dev`, Nbase and Nsta."""
    if pairs is None:
        raise ValueError("beam and ejones need the station-pair table "
                         "`pairs`")
    Nbase = int(Nbase) or int(pairs.shape[0])
    if pairs.dim() != 2 or pairs.shape[0] < Nbase or pairs.shape[1] != 2 \
            or Nbase < 1:
        raise ValueError("pairs must be [Nbase, 2]")
    if R % Nbase:
        raise ValueError(f"{R} rows are no whole timeslots of {Nbase} "
                         "baselines")
    T = R // Nbase
    # the range is remembered per tensor object: ask for the caller's own
    # table where all of it is read
    lo, hi = _pair_range(pairs if pairs.shape[0] == Nbase
                         else pairs[:Nbase])
    pairs = pairs[:Nbase].to(device=dev, dtype=torch.int32).contiguous()
    N = Nsta
    kw = {}
    if beam is not None:
        if beam.dim() != 4:
            raise ValueError("beam must be [F, T, K, N], got "
                             f"{tuple(beam.shape)}")
        if N is None:
            N = int(beam.shape[3])
        if tuple(beam.shape[:2]) != (F, T) or int(beam.shape[3]) != N:
            raise ValueError(f"beam must be [{F}, {T}, K, {N}], got "
                             f"{tuple(beam.shape)}")
        if beam.shape[2] < K:
            raise ValueError(f"beam covers {beam.shape[2]} sources, the "
                             f"pack has {K}")
        kw['beam'] = beam.to(device=dev, dtype=torch.float32).contiguous()
    if ejones is not None:
        if ejones.dim() == 5:                # [F, T, K, 2, 2]: one pattern
            ejones = ejones.unsqueeze(3)
        if ejones.dim() != 6 or tuple(ejones.shape[4:]) != (2, 2):
            raise ValueError("ejones must be [F, T, K, NE, 2, 2] or "
                             f"[F, T, K, 2, 2], got {tuple(ejones.shape)}")
        Ke, NE = int(ejones.shape[2]), int(ejones.shape[3])
        if tuple(ejones.shape[:2]) != (F, T):
            raise ValueError(f"ejones must be [{F}, {T}, K, NE, 2, 2], got "
                             f"{tuple(ejones.shape)}")
        if Ke < K:
            raise ValueError(f"ejones covers {Ke} sources, the pack has {K}")
        if beam is not None and int(beam.shape[2]) != Ke:
            raise ValueError("beam and ejones disagree on [T, K]")
        if N is None:
            N = NE if NE != 1 else hi + 1
        if NE not in (1, N):
            raise ValueError(f"ejones holds {NE} patterns per source; must "
                             f"be 1 or the station count {N}")
        kw['ejones'] = ejones.to(device=dev,
                                 dtype=torch.complex64).contiguous()
    if hi >= N or (lo < 0 and not negative_ok):
        raise ValueError(f"pairs name stations {lo}..{hi}, outside the "
                         f"{N} stations of the beam buffers")
    return dict(kw, pairs=pairs, Nbase=Nbase, Nsta=N)


def predict_coh_channels(pack, u, v, w, freqs, freq0, fdelta, tdelta, dec0,
                         reduce=None, beam=None, ejones=None, pairs=None,
                         Nbase=0):
    """Coherencies of every channel of `freqs` in one launch
    (k_predict_coh_mf): [F, M, R, 2, 2] complex64, channel f equal to
    predict_coh at freqs[f] (bit for bit on point sources; an extended
    source's envelope may round differently). reduce='mean' returns their
    mean over the channels [M, R, 2, 2] instead (k_predict_coh_mean) and
    never stores the channels; it needs at least one. fdelta is the width
    of one channel.

    Optional station beam, per channel: `beam` [F, T, K, N] real gains
    (beams.station_beam_gains) and/or `ejones` [F, T, K, NE, 2, 2] complex
    patterns, NE = 1 or N, or [F, T, K, 2, 2] (what
    beams.element_jones_channels returns) for NE = 1, with `pairs`
    [Nbase, 2] and rows r = t * Nbase + b. Channel f is then predict_coh at
    freqs[f] with beam[f] and ejones[f]: the _bm kernels with gains alone,
    the _ej kernels with patterns. With neither the call is what it was
    without these arguments.

    A pack with shapelet sources raises ValueError. Empty freqs or no rows
    return an empty tensor without a launch. Once the pack and the flux
    stack of this frequency tuple are on the device, and after the first
    call with a new pair table (whose index range is read back), the path
    has no host synchronisation."""
    if reduce not in (None, 'mean'):
        raise ValueError(f"reduce must be None or 'mean', got {reduce!r}")
    gp = _mf_pack(pack, u.device, 'predict_coh_channels')
    freqs = [float(f) for f in freqs]
    F, R = len(freqs), int(u.shape[0])
    if reduce == 'mean' and F == 0:
        raise ValueError("the mean over no channels is undefined")
    if F == 0 or R == 0:
        shape = (gp.M, R, 2, 2) if reduce else (F, gp.M, R, 2, 2)
        return torch.empty(shape, dtype=torch.complex64, device=u.device)
    bm = {}
    if beam is not None or ejones is not None:
        bm = _check_beam_channels(beam, ejones, pairs, Nbase, F, R, gp.K,
                                  u.device)
    out = _ext().predict_coh_channels(
        *_mf_source_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0),
        mean=reduce == 'mean', **bm)
    return out.view(*out.shape[:-1], 2, 2)


def residuals_multifreq(pack, x, u, v, w, freqs, freq0, fdelta, tdelta, dec0,
                        J, chunk_tab, pairs, subtract=None, beam=None,
                        ejones=None):
    """x[f] - sum over subtracted clusters of J_p C_f J_q^H for every
    channel in one launch (k_residual_mf); the coherencies C_f are those of
    predict_coh_channels, with the station beam of `beam` [F, T, K, N]
    and/or `ejones` [F, T, K, NE, 2, 2] or [F, T, K, 2, 2] when given
    (k_residual_mf_bm / _ej; N is J's station count), and are never stored. x [F, R, 2, 2] complex; J
    [Mt, N, 2, 2] packed solutions; chunk_tab [M, T] global chunk id of each
    (cluster, timeslot), chunk_off[ci] included; pairs [Nbase, 2] stations
    of the baselines, R = T * Nbase; subtract [M] booleans, False for a
    cluster that is solved but stays in the residual (negative cluster id,
    residual.c:74), default all True. A row whose pair has a negative entry
    keeps x and looks up no beam. Returns [F, R, 2, 2] complex64. The first call with a new pair
    or chunk table reads its index range back for the bounds check; after
    that, and once pack and flux stack are on the device, the path has no
    host synchronisation."""
    dev = u.device
    gp = _mf_pack(pack, dev, 'residuals_multifreq')
    freqs = [float(f) for f in freqs]
    F, R = len(freqs), int(u.shape[0])
    if x.dim() != 4 or tuple(x.shape) != (F, R, 2, 2):
        raise ValueError(f"x must be [{F}, {R}, 2, 2], got {tuple(x.shape)}")
    if F == 0 or R == 0:
        return torch.empty((F, R, 2, 2), dtype=torch.complex64, device=dev)
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2):
        raise ValueError("J must be [Mt, N, 2, 2]")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if chunk_tab.dim() != 2 or chunk_tab.shape[0] != gp.M:
        raise ValueError(f"chunk_tab must be [{gp.M}, T]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 \
            or chunk_tab.shape[1] * pairs.shape[0] != R:
        raise ValueError("pairs must be [Nbase, 2] with T * Nbase rows")
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    chunk_tab, pairs = i32(chunk_tab), i32(pairs)
    # the kernel indexes J by both tables with no checks of its own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of J")
    lo, hi = _pair_range(chunk_tab)
    if lo < 0 or hi >= Mt:
        raise ValueError(f"chunk_tab names chunks {lo}..{hi}, J has {Mt}")
    skip = None
    if subtract is not None:
        sub = torch.as_tensor(subtract).to(torch.bool)
        if tuple(sub.shape) != (gp.M,):
            raise ValueError(f"subtract must be [{gp.M}]")
        skip = (~sub).to(device=dev, dtype=torch.int32).contiguous()
    bm = {}
    if beam is not None or ejones is not None:
        bm = _check_beam_channels(beam, ejones, pairs, 0, F, R, gp.K, dev,
                                  negative_ok=True, Nsta=N)
        bm = {k: bm[k] for k in ('beam', 'ejones', 'Nsta') if k in bm}
    out = _ext().residuals_multifreq(
        x.to(torch.complex64).reshape(F, R, 4).contiguous(),
        *_mf_source_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0),
        J.to(torch.complex64).reshape(Mt, N, 4).contiguous(), chunk_tab,
        pairs, skip, **bm)
    return out.view(F, R, 2, 2)


def _beam_geometry_args(elem, nelem, du, below):
    """Checks the arguments array_beam_gains and station_beam_gains share
    and returns them as the extension wants them: (elem float64, nelem
    int32, du float64, below uint8), contiguous on elem's device."""
    import numpy as np
    if not torch.is_tensor(elem) or not elem.is_cuda:
        raise ValueError("elem must be a device tensor [N, Emax, 3]")
    if elem.dim() != 3 or elem.shape[2] != 3 or elem.shape[1] < 1:
        raise ValueError("elem must be [N, Emax, 3]")
    dev = elem.device
    N, Emax = int(elem.shape[0]), int(elem.shape[1])
    ne = np.asarray(nelem.cpu() if torch.is_tensor(nelem) else nelem)
    if ne.shape != (N,):
        raise ValueError(f"nelem must be [{N}]")
    if (ne < 1).any() or (ne > Emax).any():
        raise ValueError("every station needs 1 <= nelem <= Emax elements, "
                         f"got {ne.tolist()}")
    du = torch.as_tensor(du)
    below = torch.as_tensor(below)
    if du.dim() != 3 or du.shape[2] != 3 \
            or tuple(below.shape) != tuple(du.shape[:2]):
        raise ValueError("du must be [T, K, 3] and below [T, K]")
    return (elem.to(torch.float64).contiguous(),
            torch.as_tensor(ne.astype(np.int32)).to(dev),
            du.to(device=dev, dtype=torch.float64).contiguous(),
            below.to(device=dev, dtype=torch.uint8).contiguous())


def array_beam_gains(elem, nelem, du, below, freq):
    """Station array-factor gains on the device (k_array_beam):
      gain[t,k,n] = below[t,k] ? 0
                  : |(1/nelem[n]) sum_e exp(i 2 pi f/c elem[n,e] . du[t,k])|
    elem [N, Emax, 3] float64 ENU offsets, zero-padded, on the device the
    gains are wanted on; nelem [N] element counts, each >= 1; du [T, K, 3]
    float64 source minus pointing direction; below [T, K] bool/uint8.
    Returns [T, K, N] float32, the `beam` argument of predict_coh."""
    from ..constants import C_LIGHT
    return _ext().array_beam_gains(
        *_beam_geometry_args(elem, nelem, du, below),
        2.0 * math.pi * float(freq) / C_LIGHT)


def station_beam_gains(elem, nelem, du, below, freqs, tile=None,
                       du_tile=None):
    """Station beam gains at F frequencies in one launch (k_station_beam),
    single-stage or, with `tile` and `du_tile`, two-stage (HBA):
      gain[f,t,k,n] = below[t,k] ? 0
        : |(1/nelem[n]) sum_e exp(i 2 pi f/c elem[n,e] . du[t,k])|
          * |(1/D) sum_d exp(i 2 pi f/c tile[n,d] . du_tile[t,k])|
    elem, nelem, du, below as for array_beam_gains (elem then holds the tile
    centroids); freqs [F] Hz; tile [N, D, 3] float64 dipole offsets inside
    a tile, 1 <= D <= 64, on elem's device; du_tile [T, K, 3] source minus
    tile pointing direction. Returns [F, T, K, N] float32; row f is
    the `beam` argument of predict_coh at freqs[f]."""
    import numpy as np
    from ..constants import C_LIGHT
    elem, ne, du, below = _beam_geometry_args(elem, nelem, du, below)
    dev, N = elem.device, int(elem.shape[0])
    fq = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if fq.ndim != 1 or fq.size < 1:
        raise ValueError("freqs must be [F], F >= 1")
    if (tile is None) != (du_tile is None):
        raise ValueError("tile and du_tile are given together or not at all")
    kw = {}
    if tile is not None:
        if not torch.is_tensor(tile) or tile.device != dev:
            raise ValueError("tile must be a tensor on elem's device")
        if tile.dim() != 3 or tuple(tile.shape[::2]) != (N, 3) \
                or not 1 <= tile.shape[1] <= 64:
            raise ValueError(f"tile must be [{N}, D, 3] with 1 <= D <= 64")
        du_tile = torch.as_tensor(du_tile)
        if tuple(du_tile.shape) != tuple(du.shape):
            raise ValueError("du_tile must have du's shape [T, K, 3]")
        kw = dict(
            tile=tile.to(torch.float64).contiguous(),
            du_tile=du_tile.to(device=dev, dtype=torch.float64).contiguous())
    return _ext().station_beam_gains(
        elem, ne, du, below,
        torch.as_tensor(2.0 * math.pi * fq / C_LIGHT).to(dev), **kw)


def element_jones(coeffs, az, el, freqs, device=None):
    """Dipole element E-Jones on the device at F frequencies in one launch
    (k_element_beam). coeffs: a beams.LofarElementCoeffs; az, el: arrays or
    tensors of equal shape S (rad); freqs [F] Hz, F >= 1. The coefficient
    rows come from coeffs.at_freq in fp64 on the host (clamped at the table
    edges, interpolated inside), so only the pattern sum runs on the
    device. Returns [F, *S, 2, 2] complex64 laid out as
    LofarElementCoeffs.eval: row 0 the X dipole (Etheta, Ephi), row 1 the Y
    dipole, all four entries exactly zero where el < 0 (compared in fp64).
    `device`: where to evaluate; by default the device of az if that is a
    device tensor, else the current one."""
    import numpy as np
    ext = _ext()
    M = int(coeffs.M)
    if not 1 <= M <= ext.ELEMENT_BEAM_MAX_M:   # the kernel's unroll cap
        raise ValueError(f"the element-beam kernel takes 1 <= M <= "
                         f"{ext.ELEMENT_BEAM_MAX_M}, the table has M = {M}")
    nm = M * (M + 1) // 2
    theta, phi = np.asarray(coeffs.theta), np.asarray(coeffs.phi)
    pre = np.asarray(coeffs.preamble)
    if theta.ndim != 2 or theta.shape[1] != nm or phi.shape != theta.shape \
            or pre.shape != (nm,):
        raise ValueError(f"M = {M} needs coefficient arrays of width {nm}, "
                         f"got theta {theta.shape}, phi {phi.shape}, "
                         f"preamble {pre.shape}")
    if not float(coeffs.beta) > 0.0:
        raise ValueError("beta must be positive")
    fq = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if fq.ndim != 1 or fq.size < 1:
        raise ValueError("freqs must be [F], F >= 1")
    if device is None:
        device = az.device if torch.is_tensor(az) and az.is_cuda else 'cuda'
    az = torch.as_tensor(az)
    el = torch.as_tensor(el)
    if az.shape != el.shape:
        raise ValueError(f"az {tuple(az.shape)} and el {tuple(el.shape)} "
                         "must have one shape")
    coef = np.empty((fq.size, 2, nm), dtype=np.complex64)
    for i, f in enumerate(fq):
        coef[i, 0], coef[i, 1] = coeffs.at_freq(float(f))
    prep = lambda x: x.to(device=device,
                          dtype=torch.float64).contiguous().reshape(-1)
    E = ext.element_jones(
        prep(az), prep(el), torch.from_numpy(coef).to(device),
        torch.from_numpy(pre.astype(np.float32)).to(device), M,
        float(coeffs.beta))
    return E.view(fq.size, *az.shape, 2, 2)


class BaselineLayout:
    """Row-structure descriptor for the solver kernels: rows are
    seg*(T*Nbase) + t*Nbase + b with a fixed pair table. Built once per
    tile. pairs[b] = (p, q) as the data stores them, in any order and
    with either station first; pidx[min(p,q), max(p,q)] = b.

    The pair-index table is cached per (N, Nbase, device) and reused only
    by a layout that agrees with it on every unflagged pair, so a table
    that differs from the cached one by flagged (-1) rows alone shares it
    (the kernels skip those slots through `pairs`); any other pair order
    gets a table of its own, which takes the cache slot. The comparison
    reads the pair table back to the host, so its outcome is remembered
    per bb tensor: building the layout of the same rows again, as
    lbfgs_cost_grad does on every call, costs no synchronisation."""

    def __init__(self, bb, Nbase, T, nseg, N, device):
        self.Nbase, self.T, self.nseg, self.N = Nbase, T, nseg, N
        try:
            mkey = (dispatch.obj_token(bb), bb._version, Nbase, N,
                    str(device))
        except RuntimeError:             # inference tensor: no version
            mkey = None
        hit = _layout_memo.get(mkey)
        if hit is None:
            pairs = bb[:Nbase].to(device=device,
                                  dtype=torch.int32).contiguous()
            hit = (pairs, self._pidx_for(pairs, Nbase, N, device))
            if mkey is not None:
                if len(_layout_memo) > 64:   # bound long multi-MS runs
                    _layout_memo.pop(next(iter(_layout_memo)))
                _layout_memo[mkey] = hit
        self.pairs, self.pidx = hit

    @staticmethod
    def _pidx_for(pairs, Nbase, N, device):
        pcpu = pairs.cpu().long()
        ok = (pcpu[:, 0] >= 0) & (pcpu[:, 1] >= 0)
        lo = torch.minimum(pcpu[:, 0], pcpu[:, 1])[ok]
        hi = torch.maximum(pcpu[:, 0], pcpu[:, 1])[ok]
        b = torch.arange(Nbase, dtype=torch.int32)[ok]
        key = (N, Nbase, str(device))
        cached = _pidx_cache.get(key)
        if cached is not None and bool((cached[0][lo, hi] == b).all()):
            return cached[1]
        pidx = torch.full((N, N), -1, dtype=torch.int32)
        pidx[lo, hi] = b
        _pidx_cache[key] = (pidx, pidx.to(device).contiguous())
        return _pidx_cache[key][1]

    def chunk_tab(self, chunk_rows):
        """Per-(seg,t) global chunk id from per-row chunk indices."""
        if chunk_rows is None:
            return torch.zeros(self.nseg * self.T, dtype=torch.int32,
                               device=self.pairs.device)
        return chunk_rows[::self.Nbase].to(torch.int32).contiguous()


def _c64(t):
    return t.to(torch.complex64).reshape(t.shape[0], 4).contiguous()


def jtj_jtr(x, coh, J, bb, N, weights=None, chunk_rows=None, nchunk=1,
            layout=None):
    if layout is None:
        raise RuntimeError("GPU jtj_jtr requires a BaselineLayout "
                           "(structured rows); got none")
    ct = layout.chunk_tab(chunk_rows)
    w32 = weights.to(torch.float32).contiguous() if weights is not None \
        else None
    Jc = J.to(torch.complex64).reshape(-1, 4).contiguous()
    JtJ, Jtr, cost = _ext().jtj_jtr(
        _c64(x), _c64(coh), Jc, layout.pairs, ct, layout.pidx, w32,
        layout.Nbase, layout.T, N, layout.nseg, nchunk)
    return JtJ, Jtr, cost.sum()


def model_cost_per_chunk(x, coh, J, bb, N, weights=None, chunk_rows=None,
                         nchunk=1, layout=None):
    ct = layout.chunk_tab(chunk_rows)
    w32 = weights.to(torch.float32).contiguous() if weights is not None \
        else None
    Jc = J.to(torch.complex64).reshape(-1, 4).contiguous()
    return _ext().model_cost(_c64(x), _c64(coh), Jc, layout.pairs, ct, w32,
                             layout.Nbase, layout.T, N, layout.nseg, nchunk)


def apply_jones(coh, J, bb, chunk_rows=None, layout=None):
    if layout is None:
        # fall back to torch complex math on GPU (cold path)
        from . import reference as R
        return R.apply_jones(coh, J, bb, chunk_rows)
    ct = layout.chunk_tab(chunk_rows)
    Jc = J.to(torch.complex64).reshape(-1, 4).contiguous()
    cohs = _c64(coh).unsqueeze(0)
    out = _ext().apply_jones(None, cohs.reshape(-1, 4), Jc, layout.pairs,
                             ct, layout.Nbase, layout.T, J.shape[1],
                             layout.nseg, 1, 0)
    return out.view(-1, 2, 2)



def lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks, bb, T, Nbase,
                    robust_nu=None, weights=None):
    """Full-parameter cost/gradient on GPU via the grad-only accumulation
    kernel: r = x - sum_ci V_ci (fused residual kernel), then per cluster
    Jtr with x := r + V_ci (so the kernel's internal residual IS the total
    residual); robust scale folded as per-baseline weights. Falls back to
    the torch path when the row structure is absent."""
    from . import reference as R
    B = x.shape[0]
    M = cohs.shape[0]
    N = J_packed.shape[1]
    Mt = J_packed.shape[0]
    dev = x.device
    if B % Nbase != 0 or (B // Nbase) != T:
        return R.lbfgs_cost_grad(x, cohs, J_packed, chunk_off, nchunks,
                                 bb, T, Nbase, robust_nu, weights)
    lay = BaselineLayout(bb, Nbase, T, 1, N, dev)
    ext = _ext()
    Jc = J_packed.to(torch.complex64).reshape(-1, 4).contiguous()
    # per-cluster chunk tables (global chunk ids)
    cts = []
    Vs = []
    Vtot = torch.zeros(B, 4, dtype=torch.complex64, device=dev)
    cohs4 = cohs.to(torch.complex64).reshape(M, B, 4)
    for ci in range(M):
        rows = R.chunk_rows_for(ci, nchunks, T, Nbase, B, dev)
        if rows is None:
            rows = torch.zeros(B, dtype=torch.long, device=dev)
        rows = rows + chunk_off[ci]
        ct = rows[::Nbase].to(torch.int32).contiguous()
        cts.append(ct)
        V = ext.apply_jones(None, cohs4[ci].contiguous(), Jc, lay.pairs,
                            ct, Nbase, T, N, 1, 1, 0)
        Vs.append(V)
        Vtot += V
    x4 = x.to(torch.complex64).reshape(B, 4)
    rtot = x4 - Vtot
    e2 = (rtot.abs() ** 2).sum(dim=1)
    if robust_nu is not None:
        cost = torch.log1p(e2 / robust_nu).sum()
        scale = (1.0 / (robust_nu + e2)).to(torch.float32).contiguous()
    else:
        cost = e2.sum()
        scale = None
    grad = torch.zeros(Mt * N, 4, dtype=torch.complex64, device=dev)
    for ci in range(M):
        xsub = (rtot + Vs[ci]).contiguous()
        gci, _ = ext.jtr_grad(xsub, cohs4[ci].contiguous(), Jc, lay.pairs,
                              cts[ci], lay.pidx, scale, Nbase, T, N, 1, Mt)
        grad += gci
    g = -2.0 * torch.view_as_real(grad).reshape(-1)
    return cost.to(torch.float32), g


_chol_scratch = {}


def chol_solve_damped(JtJ, Jtr, mu):
    """dp = (JtJ + mu I)^-1 Jtr via the fused gfx950 kernel (no A
    materialization, no rocSOLVER). Failed factorizations return NaN rows
    so the LM accept mask rejects them. n is padded to a multiple of 32
    with identity diagonal (kernel requires it; pad solutions are 0)."""
    n = JtJ.shape[1]
    npad = (n + 31) // 32 * 32
    if npad != n:
        batch = JtJ.shape[0]
        J2 = torch.zeros(batch, npad, npad, dtype=JtJ.dtype,
                         device=JtJ.device)
        J2[:, :n, :n] = JtJ
        J2.diagonal(dim1=1, dim2=2)[:, n:].fill_(1.0)
        b2 = torch.zeros(batch, npad, dtype=Jtr.dtype, device=Jtr.device)
        b2[:, :n] = Jtr
        JtJ, Jtr = J2, b2
    key = (tuple(JtJ.shape), str(JtJ.device))
    sc = _chol_scratch.get(key)
    want = (JtJ.shape[0], 2 * JtJ.shape[1] * JtJ.shape[2])
    if sc is None or tuple(sc.shape) != want:
        if len(_chol_scratch) > 8:   # bound long multi-config runs
            _chol_scratch.pop(next(iter(_chol_scratch)))
        sc = torch.empty(want, dtype=JtJ.dtype, device=JtJ.device)
        _chol_scratch[key] = sc
    # n >= 384: multi-workgroup right-looking path — the trailing-update
    # SYRK tiles spread over the whole chip instead of 1 WG/problem
    # (65% of step time at [5,512,512]; see profiles/). Small n stays on
    # the single fused kernel (lower launch count wins).
    mw = os.environ.get('SAGECAL_CHOL_MW')
    use_mw = (JtJ.shape[1] >= 384) if mw is None else mw == '1'
    if use_mw:
        # chunked panels (round 2) support up to n=4096
        assert JtJ.shape[1] <= 4096, "mw Cholesky supports n <= 4096"
        dp, info = _ext().chol_solve_mw(JtJ.contiguous(), Jtr.contiguous(),
                                        mu.to(torch.float32).contiguous(),
                                        sc)
    else:
        dp, info = _ext().chol_solve(JtJ.contiguous(), Jtr.contiguous(),
                                     mu.to(torch.float32).contiguous(),
                                     sc)
    # failed factorizations already return NaN rows (kernel poisons dp)
    return dp[:, :n]
