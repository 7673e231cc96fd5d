"""Reference of the synchrosqueezed STFT and the reassignment fields (pyfft_amd.reassign, engine.ssq / ssq_bands / ssq_sum): a float64
numpy restatement of the definitions, and a float32 restatement with the same arithmetic in complex64 (a radix-2 transform written
out here, so that it rounds in float32 whatever numpy's own transform does).

    frame g = the n samples from first + g hop on, zero outside the record;  c = n / 2
    X_h, X_d, X_t = DFT(h frame), DFT(dh frame), DFT(th frame)
    khat = k - (n / 2 pi) Im(X_d conj X_h) / |X_h|^2,   gd = Re(X_t conj X_h) / |X_h|^2   (that = first + g hop + c + gd)
    Xc = (-1)^k X_h,   used = |X_h| > max(gamma, rel max_k |X_h|)
    T[g, m] = sum over the used k with rint(khat) = m of Xc,   P[g, m] = the same sum of |X_h|^2
Source bins: 0 .. n - 1 (complex records, targets modulo n, cells with |khat| >= 2^30 dropped) or 0 .. n / 2 (real records, targets
outside 0 .. n / 2 dropped).

Rounding and thresholds are discontinuous, so every coefficient is also classed as sure or UNSURE.  With
    d1 = (n / 2 pi) eps32 max_k |X_h| (1 + |X_d / X_h|) / |X_h|            (eps32 = 2^-23)
a coefficient is unsure where khat lies within KAPPA d1 of a half-integer (its target may be either neighbour; in general every
integer in rint(khat -+ KAPPA d1)), or where |X_h| lies within a factor 1 +- DELTA_T of the threshold (it may enter or leave), or,
for a band sum, where khat lies within KAPPA d1 of an edge.

KAPPA and DELTA_T were measured with measure_constants() below (python tests/ssq_ref.py): the smallest values for which the float32
restatement moves no sure coefficient of the float64 one, over every case of CASES with the noise seeds 0 .. 3, times 4:
    measured kappa = 1.57 (case n2048-hop37-first-1024-c64-band), measured delta_t = 1.45e-06 (the same case)
"Moves" is read for the fields as well as for the targets: no used khat moves by more than kappa d1 and no gd by more than kappa d1t
(d1 with th in place of dh), so that one kappa serves the squeeze and the fields.  Counting only changed targets gives 8e-4, which is
no bound on anything: few coefficients of a table this small lie that close to a half-integer.
"""
import math

import numpy as np

EPS32 = 2.0 ** -23
KAPPA_MEASURED, DELTA_T_MEASURED = 1.57, 1.45e-06
KAPPA, DELTA_T = 4 * KAPPA_MEASURED, 4 * DELTA_T_MEASURED
NFRAMES = 37

# the GPU table: the smallest shapes at which the kernel changes form (n = 32: many groups per workgroup; 4096: one group per
# workgroup; 8192: real records only), hops 1, 37 and n / 4, first = 0 and -n / 2, 37 frames so that runs and rounds do not divide, real
# and complex records, the full band and a band that drops targets (band = (b0, nb), wrapping for the complex case at 256)
CASES = [
    dict(n=32, hop=1, first=-16, cplx=False, band=None),
    dict(n=32, hop=37, first=0, cplx=True, band=None),
    dict(n=256, hop=37, first=0, cplx=False, band=(20, 40)),
    dict(n=256, hop=64, first=-128, cplx=True, band=(230, 60)),
    dict(n=256, hop=1, first=-128, cplx=False, band=None),
    dict(n=2048, hop=512, first=0, cplx=False, band=None),
    dict(n=2048, hop=37, first=-1024, cplx=True, band=(100, 700)),
    dict(n=4096, hop=1, first=-2048, cplx=False, band=None),
    dict(n=4096, hop=1024, first=0, cplx=True, band=(300, 1000)),
    dict(n=8192, hop=37, first=0, cplx=False, band=None),
    dict(n=8192, hop=2048, first=-4096, cplx=False, band=(500, 1500)),
    dict(n=256, hop=1, first=-128, cplx=True, band=None),
    dict(n=2048, hop=1, first=0, cplx=False, band=(200, 600)),
]
REL = 2e-3                # the threshold of the table: a cell is used above 2e-3 of its frame's largest


def case_id(c):
    return "n%d-hop%d-first%d-%s-%s" % (c["n"], c["hop"], c["first"], "c64" if c["cplx"] else "f32", "band" if c["band"] else "full")


def case_nsig(c):
    n, hop = c["n"], c["hop"]
    return max((NFRAMES - 1) * hop + (n if c["first"] == 0 else 1), n + 11)


def hann_windows(n):
    """periodic Hann and its exact derivative, th = (j - n / 2) h, in float64"""
    j = np.arange(n)
    t = 2 * math.pi * j / n
    h = 0.5 - 0.5 * np.cos(t)
    return h, (math.pi / n) * np.sin(t), (j - n / 2.0) * h


def make_signal(c, seed=1):
    """a chirp, a tone and 0.2 % of noise (complex for complex cases), float32-representable"""
    n, nsig = c["n"], case_nsig(c)
    rng = np.random.default_rng(1000 * seed + n + c["hop"])
    t = np.arange(nsig, dtype=np.float64)
    f0, f1 = 0.11, 0.19
    ph_c = 2 * math.pi * (f0 * t + 0.5 * (f1 - f0) / nsig * t * t)
    ph_t = 2 * math.pi * (0.31 + 0.013 / 3) * t + 0.4
    if c["cplx"]:
        x = np.exp(1j * ph_c) + 0.6 * np.exp(-1j * ph_t) + 0.002 * (rng.standard_normal(nsig) + 1j * rng.standard_normal(nsig))
        return x.astype(np.complex64)
    x = np.cos(ph_c) + 0.6 * np.cos(ph_t) + 0.002 * rng.standard_normal(nsig)
    return x.astype(np.float32)


def frames_of(x, n, hop, first, nframes, segmean=False):
    """[nframes, n]: the frames of a 1-D record, zero outside it; segmean: every frame's own mean (over its n values) removed"""
    x = np.asarray(x)
    idx = first + hop * np.arange(nframes)[:, None] + np.arange(n)[None, :]
    ok = (idx >= 0) & (idx < x.shape[0])
    fr = np.where(ok, x[np.clip(idx, 0, x.shape[0] - 1)], 0)
    if segmean:
        fr = fr - fr.mean(axis=1, keepdims=True)
    return fr


def fft32(a):
    """the DFT along the last axis with every operation rounded to complex64: radix 2, decimation in time"""
    a = np.asarray(a, dtype=np.complex64)
    n = a.shape[-1]
    bits = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    lead = a.shape[:-1]
    a = a[..., rev]
    m = 1
    while m < n:
        w = np.exp(-1j * math.pi * np.arange(m) / m).astype(np.complex64)
        a = a.reshape(lead + (n // (2 * m), 2, m))
        e, o = a[..., 0, :], a[..., 1, :] * w
        a = np.concatenate([e + o, e - o], axis=-1)
        m *= 2
    return a.reshape(lead + (n,))


def cells(x, h, dh, th, hop, first, nframes, gamma=0.0, rel=0.0, segmean=False, prec=64):
    """The cells of every frame -> dict: Xh, Xd, Xt [G, nsrc], np = |X_h|^2, mag, mmax [G], thr [G], used, khat, gd, Xc, d1 (the
    allowance of khat at kappa = 1) and d1t (the same with th in place of dh, for gd).  prec = 32: the same arithmetic in float32."""
    x = np.asarray(x)
    n = len(h)
    cplx = np.iscomplexobj(x)
    nsrc = n if cplx else n // 2 + 1
    k = np.arange(nsrc)
    if prec == 64:
        fr = frames_of(x.astype(np.complex128 if cplx else np.float64), n, hop, first, nframes, segmean)
        Xh, Xd, Xt = (np.fft.fft(fr * w, axis=1)[:, :nsrc] for w in (h, dh, th))
        ft, c1 = np.float64, n / (2 * math.pi)
    else:
        ft = np.float32
        fr = frames_of(x.astype(np.complex64 if cplx else np.float32), n, hop, first, nframes).astype(np.complex64 if cplx else np.float32)
        if segmean:
            fr = fr - (fr.sum(axis=1, keepdims=True, dtype=fr.dtype) * ft(1.0 / n))
        h32, d32, t32 = (np.asarray(w, dtype=np.float32) for w in (h, dh, th))
        if cplx:
            Xh, Xd, Xt = (fft32(fr * w) for w in (h32, d32, t32))
        else:
            z = fft32((fr * h32) + 1j * (fr * d32).astype(np.complex64))
            zm = np.conj(z[:, (-np.arange(n)) % n])
            Xh, Xd = ((z + zm) * ft(0.5))[:, :nsrc], ((z - zm) * np.complex64(-0.5j))[:, :nsrc]
            Xt = fft32(fr * t32)[:, :nsrc]
        c1 = ft(n * 0.15915494309189535)
    with np.errstate(all="ignore"):
        np_ = (Xh.real * Xh.real + Xh.imag * Xh.imag).astype(ft)
        mag = np.sqrt(np_)
        mmax = mag.max(axis=1)
        thr = np.maximum(ft(gamma), ft(rel) * mmax)
        used = mag > thr[:, None]
        khat = (k.astype(ft) - c1 * ((Xd.imag * Xh.real - Xd.real * Xh.imag).astype(ft) / np_)).astype(ft)
        gd = ((Xt.real * Xh.real + Xt.imag * Xh.imag).astype(ft) / np_).astype(ft)
        scale = (n / (2 * math.pi)) * EPS32 * mmax[:, None].astype(np.float64) / mag.astype(np.float64)
        d1 = scale * (1 + np.abs(Xd).astype(np.float64) / mag)
        d1t = scale * (1 + np.abs(Xt).astype(np.float64) / mag)
    sign = np.where(k & 1, -1.0, 1.0).astype(ft)
    return dict(n=n, cplx=cplx, nsrc=nsrc, Xh=Xh, Xd=Xd, Xt=Xt, np=np_, mag=mag, mmax=mmax, thr=thr, used=used, khat=khat, gd=gd,
                Xc=Xh * sign, d1=d1, d1t=d1t)


def targets(c, khat=None):
    """rint(khat) as the target bin -> (m int64, ok): modulo n for complex records, inside 0 .. n / 2 for real ones"""
    khat = c["khat"] if khat is None else khat
    n = c["n"]
    with np.errstate(all="ignore"):
        mf = np.rint(khat)
        ok = np.isfinite(mf) & ((np.abs(mf) < 2.0 ** 30) if c["cplx"] else ((mf >= 0) & (mf <= n // 2)))
    m = np.where(ok, mf, 0).astype(np.int64)
    return (m % n if c["cplx"] else m), ok


def band_index(c, m, b0, nb):
    """target bin -> (index within the band, inside)"""
    j = (m - b0) % c["n"] if c["cplx"] else m - b0
    return j, (j >= 0) & (j < nb)


def classes(c, kappa=KAPPA, delta_t=DELTA_T):
    """-> (thr_unsure, round_unsure) per coefficient"""
    with np.errstate(all="ignore"):
        thr = c["thr"][:, None].astype(np.float64)
        mag = c["mag"].astype(np.float64)
        tu = (mag >= thr / (1 + delta_t)) & (mag <= thr * (1 + delta_t))
        kh = c["khat"].astype(np.float64)
        ru = np.abs(np.abs(kh - np.rint(kh)) - 0.5) <= kappa * c["d1"]
    return tu, ru & np.isfinite(kh)


def fixed_sum(vals, idx, nb, big):
    """sum of vals into nb cells by index, in the kernel's fixed point: scaled by 2^(48 - e), e the exponent of `big`, rounded to int64"""
    if not big > 0:
        return np.zeros(nb)
    e = max(math.frexp(float(big))[1] - 1, -127)
    acc = np.zeros(nb, dtype=np.int64)
    np.add.at(acc, idx, np.rint(np.ldexp(vals.astype(np.float64), 48 - e)).astype(np.int64))
    return np.ldexp(acc.astype(np.float64), e - 48)


def squeeze(c, b0=0, nb=None, kappa=KAPPA, delta_t=DELTA_T, fixed=False):
    """T, P [G, nb] and, per target cell, slackT / slackP = the sum of |Xc| / |X_h|^2 over the unsure coefficients that may enter or
    leave it, reach = the number of sure or unsure coefficients that may land there, the sure / unsure masks per coefficient, and
    edge [G] = the sum of |Xc| over the coefficients that may enter or leave the FRAME's sum: those at the threshold, and the unsure
    ones of whose candidate targets some are kept and some dropped (the ends of the band; 0 and n / 2 of a real record)."""
    n, G = c["n"], c["Xh"].shape[0]
    nb = (n if c["cplx"] else n // 2 + 1) - b0 if nb is None else nb
    tu, ru = classes(c, kappa, delta_t)
    live = c["used"] | tu
    unsure = live & (tu | ru)
    sure = c["used"] & ~unsure
    m, ok = targets(c)
    j, inside = band_index(c, m, b0, nb)
    T = np.zeros((G, nb), dtype=np.complex128)
    P = np.zeros((G, nb))
    slackT, slackP, reach = np.zeros((G, nb)), np.zeros((G, nb)), np.zeros((G, nb), dtype=np.int64)
    edge = np.zeros(G)
    thr_unsure = tu & live
    take = c["used"] & ok & inside
    for g in range(G):
        s = take[g]
        if fixed:
            big = np.max(np.maximum(np.abs(c["Xh"][g].real), np.abs(c["Xh"][g].imag)))
            T[g] = fixed_sum(c["Xc"][g][s].real, j[g][s], nb, big) + 1j * fixed_sum(c["Xc"][g][s].imag, j[g][s], nb, big)
            P[g] = fixed_sum(c["np"][g][s], j[g][s], nb, float(np.max(c["np"][g])))
        else:
            np.add.at(T[g], j[g][s], c["Xc"][g][s].astype(np.complex128))
            np.add.at(P[g], j[g][s], c["np"][g][s].astype(np.float64))
        ss = sure[g] & ok[g] & inside[g]
        np.add.at(reach[g], j[g][ss], 1)
    gs, ks = np.nonzero(unsure)
    for g, k in zip(gs, ks):
        kh, d = float(c["khat"][g, k]), kappa * float(c["d1"][g, k])
        if not math.isfinite(kh):
            continue
        if not math.isfinite(d) or d >= n:
            cand = np.arange(nb)
            leaves = not (c["cplx"] and nb == n)
        else:
            mm = np.arange(int(np.rint(kh - d)), int(np.rint(kh + d)) + 1)
            ntot = mm.size
            if c["cplx"]:
                mm = mm % n
            else:
                mm = mm[(mm >= 0) & (mm <= n // 2)]
            jj, ins = band_index(c, mm, b0, nb)
            cand = np.unique(jj[ins])
            leaves = 0 < int(ins.sum()) < ntot                # some of its targets are kept and some are dropped
        if cand.size and (leaves or thr_unsure[g, k]):
            edge[g] += float(c["mag"][g, k])
        slackT[g, cand] += float(c["mag"][g, k])
        slackP[g, cand] += float(c["np"][g, k])
        reach[g, cand] += 1
    return dict(T=T, P=P, slackT=slackT, slackP=slackP, reach=reach, sure=sure, unsure=unsure, thr_unsure=thr_unsure, edge=edge,
                b0=b0, nb=nb)


def band_sums(c, edges, kappa=KAPPA, delta_t=DELTA_T):
    """out[b, g] = the sum of Xc over the used cells with lo <= khat < hi (edges [nbands, 2] or [nbands, G, 2], in bins, compared as
    float32 like the kernel) and slack[b, g] = the sum of |Xc| over the coefficients that are unsure for that band"""
    G = c["Xh"].shape[0]
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 2:
        e = np.repeat(e[:, None, :], G, axis=1)
    e = e.astype(np.float32).astype(np.float64)
    tu, _ = classes(c, kappa, delta_t)
    out = np.zeros((e.shape[0], G), dtype=np.complex128)
    slack = np.zeros((e.shape[0], G))
    kh = c["khat"].astype(np.float64)
    d = kappa * c["d1"]
    with np.errstate(all="ignore"):
        for b in range(e.shape[0]):
            lo, hi = e[b, :, 0][:, None], e[b, :, 1][:, None]
            inb = (kh >= lo) & (kh < hi)
            near = (np.abs(kh - lo) <= d) | (np.abs(kh - hi) <= d)
            maybe = (c["used"] | tu) & (near | (tu & (kh >= lo - d) & (kh < hi + d)))
            out[b] = np.sum(np.where(c["used"] & inb & ~maybe, c["Xc"], 0), axis=1)
            slack[b] = np.sum(np.where(maybe, c["mag"], 0), axis=1)
    return out, slack


def unsure_share(c, sq):
    """the largest share of a frame's summed |X_h| (over its used or nearly used cells) that unsure coefficients hold"""
    tot = np.sum(np.where(c["used"] | sq["unsure"], c["mag"], 0), axis=1).astype(np.float64)
    uns = np.sum(np.where(sq["unsure"], c["mag"], 0), axis=1).astype(np.float64)
    return float(np.max(uns / np.where(tot > 0, tot, 1)))


def measure_constants(cases=CASES, seeds=(0, 1, 2, 3)):
    """the smallest kappa and delta_t for which the float32 restatement moves no sure coefficient of the float64 one: no used
    coefficient's target changes unless khat lies within kappa d1 of a half-integer, no khat moves by more than kappa d1 and no gd by
    more than kappa d1t (so the same allowance serves the fields), and no coefficient crosses the threshold unless |X_h| lies within
    a factor 1 +- delta_t of it"""
    kappa, dt, worst_k, worst_t = 0.0, 0.0, None, None
    for cs, seed in ((cs, seed) for cs in cases for seed in seeds):
        x = make_signal(cs, seed)
        h, dh, th = hann_windows(cs["n"])
        a = cells(x, h, dh, th, cs["hop"], cs["first"], NFRAMES, rel=REL, prec=64)
        b = cells(x, h, dh, th, cs["hop"], cs["first"], NFRAMES, rel=REL, prec=32)
        ma, oka = targets(a)
        mb, okb = targets(b, b["khat"].astype(np.float64))
        moved = a["used"] & b["used"] & ((ma != mb) | (oka != okb))
        with np.errstate(all="ignore"):
            kh = a["khat"]
            need = (0.5 - np.abs(kh - np.rint(kh))) / a["d1"]
            flip = a["used"] != b["used"]
            r = a["mag"] / a["thr"][:, None]
            needt = np.maximum(r, 1 / r) - 1
            both = a["used"] & b["used"]
            need = np.where(moved, need, 0)
            need = np.maximum(need, np.where(both, np.abs(b["khat"].astype(np.float64) - kh) / a["d1"], 0))
            need = np.maximum(need, np.where(both, np.abs(b["gd"].astype(np.float64) - a["gd"]) / a["d1t"], 0))
        if float(np.max(need)) > kappa:
            kappa, worst_k = float(np.max(need)), case_id(cs)
        if flip.any() and float(np.max(needt[flip])) > dt:
            dt, worst_t = float(np.max(needt[flip])), case_id(cs)
    return kappa, dt, worst_k, worst_t


if __name__ == "__main__":
    k_, t_, wk_, wt_ = measure_constants()
    print("measured kappa %.4g (%s), delta_t %.3g (%s)" % (k_, wk_, t_, wt_))
