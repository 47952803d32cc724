"""Host-side adapters between the dispatch API and the gfx950 kernels.

Handles layout preparation: per-frequency flux scaling (done with torch on
device, keeping the predict kernel free of spectral-index math), baking the
projection identity into unused rotation terms, the device-resident
shapelet mode table, chunk tables, station-pair index tables, and
complex64 views.
"""
import math
import os

import numpy as np
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
      entry_off          int32 [M+1]  entries of cluster ci at
                         entry_off[ci] <= s < entry_off[ci+1]; read by the
                         all-channels kernels only

    These are FIELDS, and `record` maps each name to its tensor: the `tab`
    argument of the extension's shapelet entry points, which look the
    fields up by name (SHAPELET_FIELDS in bindings.cpp).

    `float` is float32, the kernel's layout; dtype=torch.float64 keeps the
    host-computed values unrounded for fp64 checks of the mirror. The
    main-kernel rotation arrays of GPUPack bake use_proj | stype>=2, which
    is wrong for shapelets, so the table bakes its own."""

    FIELDS = ('src', 'cluster', 'n0', 'beta', 'off', 'coef', 'cxi', 'sxi',
              'cphi', 'sphi', 'psign', 'a', 'b', 'ceP', 'seP', 'll', 'mm',
              'nn1', 'rec', 'entry_off')

    def __init__(self, pack, device, dtype=torch.float32):
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
        cluster = np.searchsorted(co, src, side='right') - 1
        self.cluster = i32(cluster)
        self.entry_off = i32(np.searchsorted(cluster, np.arange(self.M + 1)))
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
        self.record = {k: getattr(self, k) for k in self.FIELDS}
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
    direction cosines, projection identity baked for use_proj=False).
    `record` maps each name of FIELDS to its tensor: the `src` argument of
    the extension's predict entry points, which look the fields up by name
    (SOURCE_FIELDS in bindings.cpp). The fluxes are [4, K] stacks of the I,
    Q, U, V rows: `flux` at freq0 and `flux0` at the catalogue f0."""

    FIELDS = ('ll', 'mm', 'nn1', 'eX', 'eY', 'eP', 'cxi', 'sxi', 'cphi',
              'sphi', 'stype', 'cluster_off')

    def __init__(self, pack, device):
        f32 = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        f64 = lambda t: t.to(device=device, dtype=torch.float64).contiguous()
        self.M = pack.M
        self.K = int(pack.cluster_off[-1])       # sources in the pack
        self.ll, self.mm, self.nn1 = f64(pack.ll), f64(pack.mm), f64(pack.nn1)
        for k in ('spec_idx', 'spec_idx1', 'spec_idx2', 'eX', 'eY', 'eP'):
            setattr(self, k, f32(getattr(pack, k)))
        stack = lambda ks: torch.stack([f32(getattr(pack, k)) for k in ks])
        self.flux = stack(('sI', 'sQ', 'sU', 'sV'))
        self.flux0 = stack(('sI0', 'sQ0', 'sU0', 'sV0'))
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
        self.sh = self._sh_flux = self._sh_flux0 = None
        if getattr(pack, 'shapelets', None):
            self.sh = ShapeletTable(pack, device)
            self._sh_flux = self.flux.index_select(1, self.sh.src)  # [4,S]
            self._sh_flux0 = self.flux0.index_select(1, self.sh.src)
            self.flux[:, self.stype == 4] = 0.0
            self.flux0[:, self.stype == 4] = 0.0
        self.pack_ref = pack
        # zero shape angles for point sources keep the envelope branch out
        self.cluster_off = pack.cluster_off.to(device=device,
                                               dtype=torch.int32).contiguous()
        self.record = {k: getattr(self, k) for k in self.FIELDS}
        self.freq0 = None
        self._flux_cache = {}    # channel -> ([4, K], [4, S] or None)
        self._stack_cache = {}   # channels -> ([F, 4, K], [F, 4, S], freqs)

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

    def _channel_fluxes(self, freq, freq0):
        """(flux [4, K], shapelet flux [4, S] or None) float32 at channel
        `freq`: within 1 Hz of freq0 the pack fluxes, else the
        spectral-index scaling of the catalogue fluxes. Remembered per
        channel."""
        key = round(float(freq), 3)
        hit = self._flux_cache.get(key)
        if hit is None:
            if abs(freq - freq0) < 1.0:
                hit = (self.flux, self._sh_flux)
            else:
                flog = self._flog(freq)
                hit = (self._scale(self.flux0, flog),
                       None if self.sh is None else self._scale(
                           self._sh_flux0, flog.index_select(0, self.sh.src)))
            self._flux_cache[key] = hit
        return hit

    def _channel_stacks(self, freqs, freq0):
        """(flux [F, 4, K], shapelet flux [F, 4, S] or None, freqs [F]
        float64) on the device: row f is _channel_fluxes(freqs[f], freq0).
        Remembered per frequency tuple."""
        key = (tuple(round(float(f), 3) for f in freqs),
               round(float(freq0), 3))
        hit = self._stack_cache.get(key)
        if hit is None:
            rows = [self._channel_fluxes(float(f), freq0) for f in freqs]
            hit = dispatch.remember(self._stack_cache, key, (
                torch.stack([r[0] for r in rows]),
                None if self.sh is None else torch.stack(
                    [r[1] for r in rows]),
                torch.tensor([float(f) for f in freqs], dtype=torch.float64,
                             device=self.ll.device)), 16)
        return hit

    def fluxes_at(self, freq, freq0):
        """Per-source fluxes (sI, sQ, sU, sV) at channel `freq`, the rows of
        a [4, K] stack; pack fluxes are given at freq0 and catalogue f0.
        Shapelet sources are zero here (shapelet_fluxes_at has theirs)."""
        return tuple(self._channel_fluxes(freq, freq0)[0])

    def shapelet_fluxes_at(self, freq, freq0):
        """Un-zeroed I, Q, U, V of the shapelet sources at channel `freq`,
        [4, S] float32 in table order."""
        return self._channel_fluxes(freq, freq0)[1]

    def flux_stack(self, freqs, freq0):
        """(fluxes [F, 4, K] float32, freqs [F] float64) on the device for
        the all-channels kernels: row f stacks fluxes_at(freqs[f], freq0)."""
        flux, _, fq = self._channel_stacks(freqs, freq0)
        return flux, fq

    def shapelet_flux_stack(self, freqs, freq0):
        """Fluxes [F, 4, S] float32 of the shapelet sources for the
        all-channels kernels: row f is shapelet_fluxes_at(freqs[f], freq0)."""
        return self._channel_stacks(freqs, freq0)[1]

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
        dispatch.remember(_gpu_pack_cache, key, GPUPack(pack, device), 16)
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
            dispatch.remember(_nsta_memo, key, hit, 64)
    return hit


def _check_ejones(ejones, beam, pairs, Nbase, R, K, dev):
    """Host-side contract of the single-channel E-Jones kernels:
    _check_beam_channels for the one channel of ejones [T, K, NE, 2, 2] and
    beam [T, K, N], with the station range taken over every row of the
    caller's `pairs`, whose answer is remembered per tensor. A beam that is
    not three-dimensional is left for the extension to refuse. Returns the
    extension's keyword arguments."""
    if ejones.dim() != 5:
        raise ValueError("ejones must be [T, K, NE, 2, 2], got "
                         f"{tuple(ejones.shape)}")
    beam3 = beam is not None and beam.dim() == 3
    kw = _check_beam_channels(beam[None] if beam3 else None, ejones[None],
                              pairs, Nbase, 1, R, K, dev, all_pairs=True)
    kw['ejones'] = kw['ejones'][0]
    if beam3:
        kw['beam'] = kw['beam'][0]
    elif beam is not None:
        kw['beam'] = beam.to(device=dev, dtype=torch.float32).contiguous()
    return kw


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
    flux, sh_flux = gp._channel_fluxes(freq, freq0)
    r1 = gp.r1_for(dec0)
    uvw = [t.to(torch.float64).contiguous() for t in (u, v, w)]
    chan = (float(freq), float(fdelta) * 0.5, float(tdelta))
    bm = {}
    if ejones is not None:
        if os.environ.get('SAGECAL_SHAPELET_HOST') == '1' \
                and gp.sh is not None:
            raise RuntimeError("the torch shapelet mirror has no E-Jones")
        bm = _check_ejones(ejones, beam, pairs, Nbase, int(u.shape[0]),
                           gp.K, u.device)
    elif beam is not None:
        Nbase = int(Nbase) or int(pairs.shape[0])
        bm = dict(
            beam=beam.to(device=u.device, dtype=torch.float32).contiguous(),
            pairs=pairs[:Nbase].to(device=u.device,
                                   dtype=torch.int32).contiguous(),
            Nbase=Nbase)
    out = _ext().predict_coh(*uvw, gp.record, flux, r1, *chan, **bm)
    if gp.sh is not None:
        tab = gp.sh
        r1s = r1.index_select(0, tab.src)
        if beam is not None and beam.shape[1] < tab.K:
            raise ValueError("beam covers fewer sources than the pack")
        if os.environ.get('SAGECAL_SHAPELET_HOST') == '1':
            # torch mirror of the kernel (same table), for cross-checks
            add = shapelet_coh_torch(
                tab, sh_flux, r1s, *uvw, float(freq), float(fdelta),
                float(tdelta), bm.get('beam'), bm.get('pairs'),
                bm.get('Nbase', 0))
            out = out + add.reshape(gp.M, -1, 4).to(out.dtype)
        else:
            _ext().shapelet_coh_add(out, *uvw, tab.record, sh_flux, r1s,
                                    *chan, **bm)
    return out.view(gp.M, -1, 2, 2)


def _mf_call_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0):
    """The per-call values of the extension's all-channels entry points, by
    name: rows (u, v, w), the flux stacks and r1 of the pack (`src`) and of
    its shapelet table (`tab`, None without one), and chan (freqs, fdelta2,
    tdelta). Device work only, no synchronisation."""
    flux, sh_flux, fq = gp._channel_stacks(freqs, freq0)
    r1 = gp.r1_for(dec0)
    return dict(
        rows=[t.to(torch.float64).contiguous() for t in (u, v, w)],
        src=(flux, r1),
        tab=None if gp.sh is None else (sh_flux,
                                        r1.index_select(0, gp.sh.src)),
        chan=(fq, float(fdelta) * 0.5, float(tdelta)))


def _mf_pack(pack, device, what, shapelets=False):
    gp = pack if isinstance(pack, GPUPack) else gpu_pack(pack, device)
    if gp.sh is not None and not shapelets:
        raise ValueError(f"{what} takes shapelet sources with "
                         "shapelets=True only; without it predict this "
                         "pack channel by channel with predict_coh")
    return gp


def _check_beam_channels(beam, ejones, pairs, Nbase, F, R, K, dev,
                         negative_ok=False, Nsta=None, all_pairs=False):
    """Host-side contract of the beamed all-channels kernels, which index
    beam [F, T, Ke, N] and ejones [F, T, Ke, NE, 2, 2] (or [F, T, Ke, 2, 2],
    one pattern, NE = 1) by channel, timeslot, source and station with no
    checks of their own. Checked once here, and through _check_ejones for
    the single-channel kernels: leading dimension F, [T, Ke] agreement,
    Ke >= K, the station range of `pairs` inside N, NE in (1, N).
    negative_ok: the residual kernels keep x on a row with a negative pair
    entry and look nothing up for it, the predict kernels have no such row.
    Nsta: the station count when the caller has one (J's), else beam's, else
    NE or the largest pair entry + 1. all_pairs: the station range of every
    row of `pairs`, not of the first Nbase alone. Returns the keyword
    arguments of the extension: beam float32, ejones complex64 six-dimensional, pairs int32 [Nbase, 2], all
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
    lo, hi = _pair_range(pairs if all_pairs or pairs.shape[0] == Nbase
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
                         Nbase=0, shapelets=False):
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

    A pack with shapelet sources raises ValueError, unless shapelets=True:
    then a second launch on the same stream (k_shapelet_coh_mf /
    k_shapelet_coh_mean, with a beam their _bm / _ej variants) adds the
    shapelet sources of every channel into the result, channel f equal to
    predict_coh at freqs[f] up to rounding, with the same beam, ejones and
    pairs and under the checks already made. SAGECAL_SHAPELET_HOST is not
    consulted on this path: there is no torch mirror of these kernels. On a
    pack without shapelet sources shapelets=True changes nothing.

    Empty freqs or no rows return an empty tensor without a launch. Once
    the pack, its mode table and the flux stacks of this frequency tuple
    are on the device, and after the first call with a new pair table
    (whose index range is read back), the path has no host
    synchronisation."""
    if reduce not in (None, 'mean'):
        raise ValueError(f"reduce must be None or 'mean', got {reduce!r}")
    gp = _mf_pack(pack, u.device, 'predict_coh_channels', shapelets)
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
    a = _mf_call_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0)
    out = _ext().predict_coh_channels(*a['rows'], gp.record, *a['src'],
                                      *a['chan'], mean=reduce == 'mean', **bm)
    if gp.sh is not None:
        _ext().shapelet_coh_channels_add(
            out, *a['rows'], gp.sh.record, *a['tab'], *a['chan'],
            mean=reduce == 'mean', K=gp.K, **bm)
    return out.view(*out.shape[:-1], 2, 2)


def residuals_multifreq(pack, x, u, v, w, freqs, freq0, fdelta, tdelta, dec0,
                        J, chunk_tab, pairs, subtract=None, beam=None,
                        ejones=None, shapelets=False):
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
    host synchronisation.

    A pack with shapelet sources raises ValueError, unless shapelets=True:
    then k_shapelet_residual_mf (or its _bm / _ej variant), launched after
    the main kernel on the same stream, subtracts J_p C_f J_q^H of the
    shapelet sources of every subtracted cluster from the result, with the
    same tables and beam. SAGECAL_SHAPELET_HOST is not consulted on this
    path; on a pack without shapelet sources shapelets=True changes
    nothing."""
    dev = u.device
    gp = _mf_pack(pack, dev, 'residuals_multifreq', shapelets)
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
    a = _mf_call_args(gp, u, v, w, freqs, freq0, fdelta, tdelta, dec0)
    J4 = J.to(torch.complex64).reshape(Mt, N, 4).contiguous()
    out = _ext().residuals_multifreq(
        x.to(torch.complex64).reshape(F, R, 4).contiguous(), *a['rows'],
        gp.record, *a['src'], *a['chan'], J4, chunk_tab, pairs, skip, **bm)
    if gp.sh is not None:
        _ext().shapelet_residuals_add(
            out, *a['rows'], gp.sh.record, *a['tab'], *a['chan'], J4,
            chunk_tab, pairs, skip, K=gp.K, **bm)
    return out.view(F, R, 2, 2)


def _beam_geometry_args(elem, nelem, du, below):
    """Checks the arguments array_beam_gains and station_beam_gains share
    and returns them as the extension wants them: (elem float64, nelem
    int32, du float64, below uint8), contiguous on elem's device."""
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
                dispatch.remember(_layout_memo, mkey, hit, 64)
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


LBFGS_TSPLIT = 32    # most timeslots of one extent of k_lbfgs_mf_grad
_lbfgs_tab_memo = {}  # (kind, table token, version, ...) -> device tables


def _table_memo(kind, table, extra, build):
    """build() once per (kind, table tensor, extra), like _pair_range."""
    try:
        key = (kind, dispatch.obj_token(table), table._version) + extra
    except RuntimeError:                 # inference tensor: no version
        return build()
    hit = _lbfgs_tab_memo.get(key)
    if hit is None:
        hit = dispatch.remember(_lbfgs_tab_memo, key, build(), 64)
    return hit


def _lbfgs_extents(chunk_tab, Mt, tsplit=LBFGS_TSPLIT):
    """(ext [E, 4], ext_off [Mt + 1]) int32 on chunk_tab's device, the walk
    plan of k_lbfgs_mf_grad and k_leverage: every cluster's row of chunk_tab
    [M, T] cut into runs of one chunk id, runs longer than tsplit cut into
    pieces of at most that; one extent (ci, c, t0, t1) per piece, sorted by chunk c
    (stable: by cluster, then time), and ext_off[c] the first extent of
    chunk c. Reads the table back, so it is built once per table."""
    def build():
        ct = chunk_tab.cpu().numpy()
        ext = []
        for ci, row in enumerate(ct):
            cuts = np.flatnonzero(np.diff(row)) + 1
            for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(row)]):
                ext += [(ci, int(row[a]), t0, min(t0 + tsplit, int(b)))
                        for t0 in range(int(a), int(b), tsplit)]
        ext = np.array(ext, dtype=np.int32).reshape(-1, 4)
        ext = ext[np.argsort(ext[:, 1], kind='stable')]
        off = np.zeros(Mt + 1, dtype=np.int32)
        off[1:] = np.cumsum(np.bincount(ext[:, 1], minlength=Mt))
        return tuple(torch.from_numpy(a).to(chunk_tab.device)
                     for a in (ext, off))
    return _table_memo('ext', chunk_tab, (Mt, tsplit), build)


def _lbfgs_stations(pairs, N):
    """(sta_off [N + 1], sta_ent) int32 on pairs' device, what
    k_lbfgs_mf_reduce sums for a station: entry 2*b + side for every pair b
    without a negative entry and side 0 (p) and 1 (q), sorted by station,
    then by entry. Reads the table back, so it is built once per table."""
    def build():
        pr = pairs.cpu().numpy()
        ok = np.flatnonzero((pr >= 0).all(axis=1))
        sta = pr[ok].reshape(-1)                    # p0, q0, p1, q1, ...
        ent = (2 * ok[:, None] + np.arange(2)).reshape(-1)
        order = np.argsort(sta, kind='stable')
        off = np.zeros(N + 1, dtype=np.int32)
        off[1:] = np.cumsum(np.bincount(sta, minlength=N))
        return tuple(torch.from_numpy(a).to(pairs.device)
                     for a in (off, ent[order].astype(np.int32)))
    return _table_memo('sta', pairs, (N,), build)


def lbfgs_cost_grad_channels(xs, cohs, J, chunk_tab, pairs, robust_nu=None):
    """Cost and gradient of the LBFGS objective summed over the channels,
    the sum over f of lbfgs_cost_grad(xs[f], cohs[f], ...), in three launches
    whatever F and M (lbfgs_mf.hip): xs [F, R, 2, 2], cohs [F, M, R, 2, 2],
    J [Mt, N, 2, 2] complex; chunk_tab [M, T] global chunk id of each
    (cluster, timeslot), chunk_off[ci] included; pairs [Nbase, 2] stations of
    the baselines, stored either way round and in any order, R = T * Nbase,
    a row whose pair has a negative entry adds nothing. Gaussian cost, or
    with robust_nu sum log1p(e2 / nu). Returns (cost [] float32, grad
    [Mt*N*8] float32 in the order of view_as_real(J)); bitwise the same from
    call to call. The first call with a new pair or chunk table reads it
    back, for the bounds check and the kernels' index tables; after that the
    path has no host synchronisation."""
    dev = xs.device
    if xs.dim() != 4 or tuple(xs.shape[2:]) != (2, 2):
        raise ValueError(f"xs must be [F, R, 2, 2], got {tuple(xs.shape)}")
    F, R = int(xs.shape[0]), int(xs.shape[1])
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2) or J.shape[0] < 1 \
            or J.shape[1] < 1:
        raise ValueError("J must be [Mt, N, 2, 2]")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if cohs.dim() != 5 or cohs.shape[0] != F \
            or tuple(cohs.shape[2:]) != (R, 2, 2):
        raise ValueError(f"cohs must be [{F}, M, {R}, 2, 2], got "
                         f"{tuple(cohs.shape)}")
    M = int(cohs.shape[1])
    if chunk_tab.dim() != 2 or chunk_tab.shape[0] != M:
        raise ValueError(f"chunk_tab must be [{M}, T]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 \
            or chunk_tab.shape[1] * pairs.shape[0] != R:
        raise ValueError("pairs must be [Nbase, 2] with T * Nbase rows")
    if robust_nu is not None and not float(robust_nu) > 0.0:
        raise ValueError("robust_nu must be positive")
    if F == 0 or R == 0 or M == 0:
        return (torch.zeros((), dtype=torch.float32, device=dev),
                torch.zeros(Mt * N * 8, dtype=torch.float32, device=dev))
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    chunk_tab, pairs = i32(chunk_tab), i32(pairs)
    # the kernels index J by both tables with no checks of their own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of J")
    lo, hi = _pair_range(chunk_tab)
    if lo < 0 or hi >= Mt:
        raise ValueError(f"chunk_tab names chunks {lo}..{hi}, J has {Mt}")
    ext, ext_off = _lbfgs_extents(chunk_tab, Mt)
    sta_off, sta_ent = _lbfgs_stations(pairs, N)

    def c64(t, *shape):
        # contiguous, and 16-byte aligned for the kernels' float4 loads (a
        # view may start 8 bytes into its storage)
        t = t.to(torch.complex64).reshape(*shape).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    cost, grad = _ext().lbfgs_cost_grad_channels(
        c64(xs, F, R, 4), c64(cohs, F, M, R, 4), c64(J, Mt, N, 4), chunk_tab,
        pairs, ext, ext_off, sta_off, sta_ent,
        0.0 if robust_nu is None else float(robust_nu))
    return cost, grad


JOINT_TT = 32        # time tile of k_joint_gram (JOINT_JTJ_TT, launchers.h)


def _joint_tables(chunk_tab, Mt, blocked):
    """The walk plan of k_joint_gram and the destinations of k_joint_reduce,
    int32 on chunk_tab's device, as the dict JointJtjArgs is filled from:
    pieces [E, 2] (the finest segments over which every cluster's chunk id
    is constant, cut at JOINT_TT timeslots, in time order), etab
    [E, M(M+1)/2] and gtab [E, M] (2*slot + first: the slot a piece adds
    to and whether it is the first to), cbin [E], sdst [D, 2], gdst [G],
    cpos [Mt, 2], with nblk and nbin. Blocked: chunk c is chunk c % Kb of
    cluster c // Kb, Kb = Mt / M, and block k holds chunk k of every
    cluster; ValueError where a timeslot mixes blocks. Reads the table
    back, so it is built once per table."""
    def build():
        ct = chunk_tab.cpu().numpy()
        M, T = ct.shape
        Kb = Mt // M
        if blocked:
            if Kb * M != Mt or (ct // Kb != np.arange(M)[:, None]).any() \
                    or (ct % Kb != ct[:1] % Kb).any():
                raise ValueError(
                    "the blocked layout needs the same chunk count and "
                    "chunk boundaries in every cluster")
            c = np.arange(Mt)
            cpos = np.stack([c % Kb, c // Kb], axis=1)
        else:
            cpos = np.stack([np.zeros(Mt, dtype=np.int64), np.arange(Mt)],
                            axis=1)
        cuts = np.flatnonzero((np.diff(ct, axis=1) != 0).any(axis=0)) + 1
        pieces = [(t0, min(t0 + JOINT_TT, int(b)))
                  for a, b in zip(np.r_[0, cuts], np.r_[cuts, T])
                  for t0 in range(int(a), int(b), JOINT_TT)]
        slots, gslots, etab, gtab = {}, {}, [], []

        def slot_of(table, key):
            first = key not in table
            return 2 * table.setdefault(key, len(table)) + first
        for t0, _ in pieces:
            col = [int(v) for v in ct[:, t0]]
            etab.append([slot_of(slots, (col[i], col[j]))
                         for i in range(M) for j in range(i, M)])
            gtab.append([slot_of(gslots, v) for v in col])
        cbin = [int(ct[0, t0]) % Kb if blocked else 0 for t0, _ in pieces]
        tabs = dict(pieces=pieces, etab=etab, gtab=gtab, cbin=cbin,
                    sdst=list(slots), gdst=list(gslots), cpos=cpos)
        out = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
               .to(chunk_tab.device) for k, v in tabs.items()}
        out['nblk'] = out['nbin'] = Kb if blocked else 1
        return out
    return _table_memo('joint', chunk_tab, (Mt, bool(blocked), JOINT_TT),
                       build)


def _joint_launch(x, cohs, J, chunk_tab, pairs, weights, blocked, cost_only):
    """Checks and launch shared by joint_jtj_jtr and joint_cost."""
    dev = x.device
    if x.dim() != 3 or tuple(x.shape[1:]) != (2, 2):
        raise ValueError(f"x must be [R, 2, 2], got {tuple(x.shape)}")
    R = int(x.shape[0])
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2) or J.shape[0] < 1 \
            or J.shape[1] < 1:
        raise ValueError("J must be [Mt, N, 2, 2]")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if cohs.dim() != 4 or cohs.shape[0] < 1 \
            or tuple(cohs.shape[1:]) != (R, 2, 2):
        raise ValueError(f"cohs must be [M, {R}, 2, 2], got "
                         f"{tuple(cohs.shape)}")
    M = int(cohs.shape[0])
    if chunk_tab.dim() != 2 or chunk_tab.shape[0] != M:
        raise ValueError(f"chunk_tab must be [{M}, T]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or R == 0 \
            or chunk_tab.shape[1] * pairs.shape[0] != R:
        raise ValueError("pairs must be [Nbase, 2] with T * Nbase rows")
    if weights is not None and tuple(weights.shape) != (R,):
        raise ValueError(f"weights must be [{R}]")
    if M > 30:
        raise ValueError("the joint kernels stage 32 timeslots of all "
                         f"clusters in LDS, at most 30 clusters; got {M}")
    if _ext().JOINT_JTJ_TT != JOINT_TT:
        raise RuntimeError("JOINT_TT differs from the kernels' time tile")
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    chunk_tab, pairs = i32(chunk_tab), i32(pairs)
    # the kernels index J by both tables with no checks of their own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of J")
    lo, hi = _pair_range(chunk_tab)
    if lo < 0 or hi >= Mt:
        raise ValueError(f"chunk_tab names chunks {lo}..{hi}, J has {Mt}")
    tb = _joint_tables(chunk_tab, Mt, blocked)
    sta_off, sta_ent = _lbfgs_stations(pairs, N)

    def c64(t, *shape):
        t = t.to(torch.complex64).reshape(*shape).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    if weights is not None:
        weights = weights.to(device=dev, dtype=torch.float32).contiguous()
    return _ext().joint_jtj(
        c64(x, R, 4), c64(cohs, M, R, 4), c64(J, Mt, N, 4), weights, pairs,
        chunk_tab, tb['pieces'], tb['etab'], tb['gtab'], tb['cbin'],
        tb['sdst'], tb['gdst'], tb['cpos'], sta_off, sta_ent, tb['nblk'],
        tb['nbin'], cost_only)


def joint_jtj_jtr(x, cohs, J, chunk_tab, pairs, weights=None, blocked=False):
    """reference.joint_jtj_jtr from the kernels of joint_jtj.hip, two
    launches: x [R, 2, 2], cohs [M, R, 2, 2], J [Mt, N, 2, 2] complex;
    chunk_tab [M, T] global chunk id of each (cluster, timeslot); pairs
    [Nbase, 2] in any order and orientation, R = T * Nbase, a pair with a
    negative entry adds nothing; weights [R] >= 0 or None. Returns float32
    (H [P, P], g [P], cost []) with P = 8 Mt N, or with blocked=True
    (H [Kb, Pb, Pb], g [Kb, Pb], cost [Kb]), Pb = 8 M N, parameter order
    (cluster, station, 8) inside block k, which holds chunk k of every
    cluster. H is symmetric bit for bit and all three repeat bit for bit
    from call to call. The first call with a new pair or chunk table reads
    it back; after that the path has no host synchronisation."""
    H, g, cost = _joint_launch(x, cohs, J, chunk_tab, pairs, weights,
                               blocked, False)
    if blocked:
        return H, g, cost
    return H[0], g[0], cost[0]


def joint_cost(x, cohs, J, chunk_tab, pairs, weights=None, blocked=False):
    """The weighted cost of joint_jtj_jtr alone at J, [] or per block [Kb]:
    the LM trial cost. No H is allocated or written."""
    cost, = _joint_launch(x, cohs, J, chunk_tab, pairs, weights, blocked,
                          True)
    return cost if blocked else cost[0]


RTR_TCG_MAXN = 512          # RTR_TCG_MAXP / 8 of launchers.h


def rtr_tcg(JtJ, Jtr, J, iw, delta, maxit=12, kappa=0.01):
    """The RTR inner solve of one outer iteration in one launch of k_rtr_tcg
    (rtr_tcg.hip), one workgroup per chunk: JtJ [n, 8N, 8N], Jtr [n, 8N],
    J [n, N, 2, 2], iw [N], delta [n] on the device, computed in float32.
    Returns (g, eta, Heta) [n, N, 2, 2] complex64, what rtr._Objective.grad,
    rtr._tcg_fixed and hess_vec(J, eta) give, and stats [n, 4] float32 =
    (<g,g>, <g,eta>, <eta,Heta>, CG iterations entered). Two calls on the
    same input agree bit for bit; no host synchronisation."""
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2) or J.shape[0] < 1:
        raise ValueError(f"J must be [n, N, 2, 2], got {tuple(J.shape)}")
    n, N = int(J.shape[0]), int(J.shape[1])
    if N < 2 or N > RTR_TCG_MAXN:
        raise ValueError(f"rtr_tcg takes 2 to {RTR_TCG_MAXN} stations "
                         f"(8 N <= {8 * RTR_TCG_MAXN}), got {N}")
    if tuple(JtJ.shape) != (n, 8 * N, 8 * N) \
            or tuple(Jtr.shape) != (n, 8 * N):
        raise ValueError(f"JtJ must be [{n}, {8 * N}, {8 * N}] and Jtr "
                         f"[{n}, {8 * N}]")
    if tuple(iw.shape) != (N,) or tuple(delta.shape) != (n,):
        raise ValueError(f"iw must be [{N}] and delta [{n}]")
    if int(maxit) < 0:
        raise ValueError("maxit must not be negative")
    dev = J.device
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    return tuple(_ext().rtr_tcg(f32(JtJ), f32(Jtr),
                                J.to(torch.complex64).contiguous(), f32(iw),
                                f32(delta), int(maxit), float(kappa)))


LEVERAGE_TSPLIT = 64  # most timeslots of one piece of k_leverage


def leverage_rows(cohs, J, Hinv, chunk_tab, pairs, weights=None):
    """The influence-map leverage of every cluster in one launch of
    k_leverage (leverage.hip): cohs [M, R, 2, 2] and J [Mt, N, 2, 2] complex,
    read as complex64, Hinv [Mt, 8N, 8N] the float64 inverse of the damped
    JtJ of every chunk, chunk_tab [M, T] global chunk id of each (cluster,
    timeslot), pairs [Nbase, 2] in any order and either way round,
    R = T * Nbase, weights [R] or None. Returns lev [M, R] float64, computed
    in float64; a row whose pair has a negative entry gets 0. Bitwise the
    same from call to call. The first call with a new pair or chunk table
    reads it back, for the bounds check and the pieces; after that the path
    has no host synchronisation."""
    dev = cohs.device
    if cohs.dim() != 4 or tuple(cohs.shape[2:]) != (2, 2):
        raise ValueError(f"cohs must be [M, R, 2, 2], got {tuple(cohs.shape)}")
    M, R = int(cohs.shape[0]), int(cohs.shape[1])
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2) or J.shape[0] < 1 \
            or J.shape[1] < 1:
        raise ValueError("J must be [Mt, N, 2, 2]")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if tuple(Hinv.shape) != (Mt, 8 * N, 8 * N):
        raise ValueError(f"Hinv must be [{Mt}, {8 * N}, {8 * N}], got "
                         f"{tuple(Hinv.shape)}")
    if chunk_tab.dim() != 2 or chunk_tab.shape[0] != M:
        raise ValueError(f"chunk_tab must be [{M}, T]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 \
            or chunk_tab.shape[1] * pairs.shape[0] != R:
        raise ValueError("pairs must be [Nbase, 2] with T * Nbase rows")
    if weights is not None and tuple(weights.shape) != (R,):
        raise ValueError(f"weights must be [{R}]")
    if M == 0 or R == 0:
        return torch.zeros(M, R, dtype=torch.float64, device=dev)
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    chunk_tab, pairs = i32(chunk_tab), i32(pairs)
    # the kernel indexes J and Hinv by both tables with no checks of its own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of J")
    lo, hi = _pair_range(chunk_tab)
    if lo < 0 or hi >= Mt:
        raise ValueError(f"chunk_tab names chunks {lo}..{hi}, J has {Mt}")
    pieces, _ = _lbfgs_extents(chunk_tab, Mt, LEVERAGE_TSPLIT)

    def c64(t, *shape):
        t = t.to(torch.complex64).reshape(*shape).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
    return _ext().leverage_rows(
        c64(cohs, M, R, 4), c64(J, Mt, N, 4), f64(Hinv),
        None if weights is None else f64(weights), chunk_tab, pairs, pieces)


NORMAL_TSPLIT = 64    # most timeslots of one piece of k_normal_accum


def _normal_pair_index(pairs, N):
    """pidx [N, N] int32 on pairs' device for k_normal_expand: 2 b at (p, q)
    and 2 b + 1 at (q, p) for every pair b = (p, q) without a negative entry,
    -1 elsewhere. A cross block belongs to one pair, so a pair named twice,
    either way round, or a pair of a station with itself raises ValueError.
    Reads the table back, so it is built once per table."""
    def build():
        pr = pairs.cpu().numpy()
        ok = np.flatnonzero((pr >= 0).all(axis=1))
        p, q = pr[ok, 0], pr[ok, 1]
        key = np.minimum(p, q).astype(np.int64) * N + np.maximum(p, q)
        if (p == q).any() or len(np.unique(key)) != len(key):
            raise ValueError("the float64 normal matrices need every pair "
                             "once and of two stations")
        idx = np.full((N, N), -1, dtype=np.int32)
        idx[p, q] = 2 * ok
        idx[q, p] = 2 * ok + 1
        return torch.from_numpy(idx).to(pairs.device)
    return _table_memo('pidx', pairs, (N,), build)


def normal_matrices(cohs, J, chunk_tab, pairs, weights=None):
    """The Gauss-Newton normal matrices JtJ [Mt, 8N, 8N] float64 of every
    chunk of every cluster in the two launches of normal_f64.hip: cohs
    [M, R, 2, 2] and J [Mt, N, 2, 2] complex, read as complex64, chunk_tab
    [M, T] global chunk id of each (cluster, timeslot), pairs [Nbase, 2] in
    any order and either way round, each pair at most once, R = T * Nbase,
    weights [R] (read as float32) or None. Every product and sum is float64;
    a pair with a negative entry adds nothing, blocks of pairs that do not
    occur and chunks that chunk_tab does not name are zero. JtJ == JtJ^T to
    the bit, and bitwise the same from call to call and in any batch. The
    first call with a new pair or chunk table reads it back, for the bounds
    check and the index tables; after that the path has no host
    synchronisation."""
    dev = cohs.device
    if cohs.dim() != 4 or tuple(cohs.shape[2:]) != (2, 2):
        raise ValueError(f"cohs must be [M, R, 2, 2], got {tuple(cohs.shape)}")
    M, R = int(cohs.shape[0]), int(cohs.shape[1])
    if J.dim() != 4 or tuple(J.shape[2:]) != (2, 2) or J.shape[0] < 1 \
            or J.shape[1] < 1:
        raise ValueError("J must be [Mt, N, 2, 2]")
    Mt, N = int(J.shape[0]), int(J.shape[1])
    if chunk_tab.dim() != 2 or chunk_tab.shape[0] != M:
        raise ValueError(f"chunk_tab must be [{M}, T]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 \
            or chunk_tab.shape[1] * pairs.shape[0] != R:
        raise ValueError("pairs must be [Nbase, 2] with T * Nbase rows")
    if weights is not None and tuple(weights.shape) != (R,):
        raise ValueError(f"weights must be [{R}]")
    zeros = lambda: torch.zeros(Mt, 8 * N, 8 * N, dtype=torch.float64,
                                device=dev)
    if M == 0 or R == 0:
        return zeros()
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    chunk_tab, pairs = i32(chunk_tab), i32(pairs)
    # the kernels index J and JtJ by both tables with no checks of their own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of J")
    lo, hi = _pair_range(chunk_tab)
    if lo < 0 or hi >= Mt:
        raise ValueError(f"chunk_tab names chunks {lo}..{hi}, J has {Mt}")
    pieces, piece_off = _lbfgs_extents(chunk_tab, Mt, NORMAL_TSPLIT)
    pidx = _normal_pair_index(pairs, N)
    sta_off, sta_ent = _lbfgs_stations(pairs, N)
    if sta_ent.numel() == 0:                 # every pair flagged
        return zeros()

    def c64(t, *shape):
        t = t.to(torch.complex64).reshape(*shape).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    if weights is not None:
        weights = weights.to(device=dev, dtype=torch.float32).contiguous()
    return _ext().normal_matrices(
        c64(cohs, M, R, 4), c64(J, Mt, N, 4), weights, chunk_tab, pairs,
        pieces, piece_off, pidx, sta_off, sta_ent)


_spd_scratch = {}


def spd_inverse_damped(JtJ, mu, return_info=False):
    """X = (JtJ + mu I)^-1 [Mt, n, n] in float64 through the kernels of
    spd_inverse.hip: JtJ [Mt, n, n] float32 or float64 on the device, read
    as symmetric from its lower triangle and left as it is, n a multiple of
    8 up to SPD_INVERSE_MAXN; mu a number or a tensor of one value or one
    per matrix. X == X^T to the bit, the same from call to call and whatever
    the batch a matrix comes in. A matrix that is not positive definite
    comes back all NaN; the flags info [Mt] int32 (non-zero: failed) stay
    on the device and come along with return_info=True as (X, info). The
    path has no host synchronisation."""
    ext = _ext()
    if JtJ.dim() != 3 or JtJ.shape[0] < 1 or JtJ.shape[1] != JtJ.shape[2]:
        raise ValueError(f"JtJ must be [Mt, n, n], got {tuple(JtJ.shape)}")
    Mt, n = int(JtJ.shape[0]), int(JtJ.shape[1])
    if n < 8 or n % 8 or n > ext.SPD_INVERSE_MAXN:
        raise ValueError(f"n must be a multiple of 8 in 8.."
                         f"{ext.SPD_INVERSE_MAXN}, got {n}")
    if JtJ.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"JtJ must be float32 or float64, got {JtJ.dtype}")
    dev = JtJ.device
    if torch.is_tensor(mu):
        mu = mu.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if mu.numel() not in (1, Mt):
            raise ValueError(f"mu must hold 1 or {Mt} values, got "
                             f"{mu.numel()}")
    else:
        mu = torch.full((1,), float(mu), dtype=torch.float64, device=dev)
    key = (Mt, n, str(dev))
    sc = _spd_scratch.get(key)
    if sc is None:
        sc = dispatch.remember(
            _spd_scratch, key,
            torch.empty(ext.spd_inverse_scratch(Mt, n), dtype=torch.float64,
                        device=dev), 4)
    A = JtJ.contiguous()
    if A.data_ptr() % 16:
        A = A.clone()
    X, info = ext.spd_inverse(A, mu, sc)
    return (X, info) if return_info else X


DIFFUSE_MAX_GZ = 4    # launchers.h
DIFFUSE_MAX_N2 = 32

_diffuse_tensors = {}


def diffuse_product_tensors(Gc, Gz, beta_c, beta_z, dev):
    """(T1 [n1, Gc, Gz], T2 [n2, Gz, n1], g2) of the two series products of
    the diffuse predict, float64 on `dev`: the Gauss-Hermite quadrature of
    shapelet.shapelet_product_tensor on the host, once per (Gc, Gz, beta_c,
    beta_z, device)."""
    from .. import shapelet
    key = (int(Gc), int(Gz), float(beta_c), float(beta_z), str(dev))
    hit = _diffuse_tensors.get(key)
    if hit is None:
        n1 = Gc + Gz - 1
        n2 = Gz + n1 - 1
        g1 = shapelet.product_scale(beta_c, beta_z)
        g2 = shapelet.product_scale(beta_z, g1)
        f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
        T1 = shapelet.shapelet_product_tensor(Gc, Gz, n1, beta_c, beta_z, g1)
        T2 = shapelet.shapelet_product_tensor(Gz, n1, n2, beta_z, g1, g2)
        hit = dispatch.remember(_diffuse_tensors, key,
                                (f64(T1), f64(T2), g2), 8)
    return hit


def diffuse_coherencies(u, v, w, pairs, T, Z, beta_z, Cm, beta_c, lmn, freq,
                        fdelta):
    """The diffuse cluster's coherencies [T * Nbase, 2, 2] complex64 through
    k_diffuse_station and k_diffuse_pair (diffuse.hip): u, v, w [T * Nbase]
    on the device, pairs [Nbase, 2] in any order and either way round, Z
    [N, Gz*Gz, 2, 2] and Cm [Gc*Gc, 2, 2] complex, read as complex128, with
    Gz <= DIFFUSE_MAX_GZ and n2 = Gc + 2 Gz - 2 <= DIFFUSE_MAX_N2. The series
    products run in float64, the mode sum in float32; a row whose pair has a
    negative entry gets zeros. Bitwise the same from call to call. The first
    call with a new pair table reads it back for the bounds check; after
    that the path has no host synchronisation."""
    dev = u.device
    if Z.dim() != 4 or tuple(Z.shape[2:]) != (2, 2) or Z.shape[0] < 1:
        raise ValueError(f"Z must be [N, Gz*Gz, 2, 2], got {tuple(Z.shape)}")
    if Cm.dim() != 3 or tuple(Cm.shape[1:]) != (2, 2):
        raise ValueError(f"Cm must be [Gc*Gc, 2, 2], got {tuple(Cm.shape)}")
    N, Gz, Gc = int(Z.shape[0]), math.isqrt(Z.shape[1]), \
        math.isqrt(Cm.shape[0])
    if Gz < 1 or Gc < 1 or Gz * Gz != Z.shape[1] or Gc * Gc != Cm.shape[0]:
        raise ValueError("Z and Cm must hold square mode grids")
    if Gz > DIFFUSE_MAX_GZ or Gc + 2 * Gz - 2 > DIFFUSE_MAX_N2:
        raise ValueError(f"the diffuse kernels take Gz <= {DIFFUSE_MAX_GZ} "
                         f"and n2 <= {DIFFUSE_MAX_N2}, got Gz = {Gz}, n2 = "
                         f"{Gc + 2 * Gz - 2}")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 \
            or int(T) < 1 or tuple(u.shape) != (int(T) * pairs.shape[0],):
        raise ValueError("pairs must be [Nbase, 2] and u [T * Nbase]")
    pairs = pairs.to(device=dev, dtype=torch.int32).contiguous()
    # the kernels index Z's operands by the table with no checks of their own
    if _pair_range(pairs)[1] >= N:
        raise ValueError(f"pairs name a station outside the {N} of Z")
    T1, T2, g2 = diffuse_product_tensors(Gc, Gz, beta_c, beta_z, dev)
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()

    def c128(t):
        t = t.to(device=dev, dtype=torch.complex128).contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()
    ll, mm, nn1 = lmn
    return _ext().diffuse_coherencies(
        f64(u), f64(v), f64(w), pairs, int(T), c128(Z), c128(Cm), T1, T2,
        float(g2), float(ll), float(mm), float(nn1), float(freq),
        0.5 * float(fdelta))


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
        sc = dispatch.remember(
            _chol_scratch, key,
            torch.empty(want, dtype=JtJ.dtype, device=JtJ.device), 8)
    # n >= 384: multi-workgroup right-looking path — the trailing-update
    # SYRK tiles spread over the whole chip instead of 1 WG/problem
    # (65% of step time at [5,512,512]; see profiles/). Small n stays on
    # the single fused kernel (lower launch count wins).
    mw = os.environ.get('SAGECAL_CHOL_MW')
    use_mw = (JtJ.shape[1] >= 384) if mw is None else mw == '1'
    if JtJ.shape[1] > 4096 and dispatch.chol_blocked_on():
        # above the mw limit: outer blocks of 128 with LDS-tiled rank-128
        # trailing updates (cholesky_blocked.hip), n <= 16384
        dp, info = _ext().chol_solve_blocked(
            JtJ.contiguous(), Jtr.contiguous(),
            mu.to(torch.float32).contiguous(), sc)
    elif use_mw:
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
