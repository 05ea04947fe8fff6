"""The variance-propagating à-trous filter's arithmetic contract ("Variance filter"),
restated in numpy float32: elementwise operations in the contract's order, nothing fused, so that
tests/test_gpu_denoise_variance.py can pin the HIP kernels bit for bit.  CPU checks of the
restatement itself and of the binding's new entry points."""
import numpy as np

import test_denoise_restate as rs

F = np.float32
H5 = rs.H5
G3 = np.array([1 / 4, 1 / 2, 1 / 4], np.float32)
VMAX = F(2.0 ** 60)
bits = rs.bits


def variance_init(avg, key, se):
    """c0: H x W x 4 = {avg.rgb, the 3x3 prefilter of min(se^2, VMAX) among the centre's key}."""
    avg = np.asarray(avg, np.float32)
    Hh, Ww = key.shape
    with np.errstate(all="ignore"):
        t = (np.asarray(se, np.float32) * np.asarray(se, np.float32)).astype(np.float32)
        vraw = np.where(t < VMAX, t, VMAX).astype(np.float32)             # NaN and +inf: VMAX
        sv = np.zeros((Hh, Ww), np.float32)
        sg = np.zeros((Hh, Ww), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                y0, y1 = max(0, -dy), min(Hh, Hh - dy)
                x0, x1 = max(0, -dx), min(Ww, Ww - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                ok = key[q] == key[p]
                gw = F(G3[dy + 1] * G3[dx + 1])
                sv[p] = np.where(ok, sv[p] + gw * vraw[q], sv[p])
                sg[p] = np.where(ok, sg[p] + gw, sg[p])
        v0 = (sv / sg).astype(np.float32)
    return np.concatenate([avg, v0[..., None]], axis=-1).astype(np.float32)


def iteration(c4, key, N, P, step, kk, kp):
    """One iteration over H x W x 4 {rgb, variance}: §3.7's taps and weights with kc from the centre's
    carried variance, the variance summed with the squared weights."""
    c4 = np.asarray(c4, np.float32)
    c, v = c4[..., :3], c4[..., 3]
    Hh, Ww = key.shape
    h22 = F(H5[2] * H5[2])
    with np.errstate(all="ignore"):
        kc = (F(1) / (F(kk) * v + F(2.0 ** -40))).astype(np.float32)
        acc = (h22 * c).astype(np.float32)
        wsum = np.full((Hh, Ww), h22, np.float32)
        vs = (F(h22 * h22) * v).astype(np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                oy, ox = step * dy, step * dx
                y0, y1 = max(0, -oy), min(Hh, Hh - oy)
                x0, x1 = max(0, -ox), min(Ww, Ww - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                kp_, kq_ = key[p], key[q]
                ok = kq_ == kp_
                cp, cq, Np, Nq, Pp, Pq = c[p], c[q], N[p], N[q], P[p], P[q]
                dc = cq - cp
                a_c = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * kc[p]
                dP = Pq - Pp
                t = (Np[..., 0] * dP[..., 0] + Np[..., 1] * dP[..., 1]) + Np[..., 2] * dP[..., 2]
                a_p = (t * t) * kp
                d = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                nd = np.where(F(0) < d, d, F(0)).astype(np.float32)
                for _ in range(5):
                    nd = nd * nd
                wn = np.where(kp_ < 0, F(1), nd).astype(np.float32)
                r = F(1) / (F(1) + (a_c + a_p))
                w = (((F(H5[dy + 2] * H5[dx + 2])) * wn) * r) * r
                assert w.dtype == np.float32 and a_c.dtype == np.float32 and a_p.dtype == np.float32
                acc[p] = np.where(ok[..., None], acc[p] + w[..., None] * cq, acc[p])
                wsum[p] = np.where(ok, wsum[p] + w, wsum[p])
                vs[p] = np.where(ok, vs[p] + (w * w) * v[q], vs[p])
        out = np.empty_like(c4)
        out[..., :3] = acc / wsum[..., None]
        out[..., 3] = vs / (wsum * wsum)
    return out


def denoise_variance4(first_input, key, N, P, se, iterations, k_color, sigma_plane):
    """H x W x 4 {rgb, variance} after `iterations`; first_input is accum / pass_count or the
    resolved colour."""
    c4 = variance_init(first_input, key, se)
    kk = F(F(k_color) * F(k_color))
    for s in range(iterations):
        step, _, kp = rs.constants(s, 1.0, sigma_plane)
        c4 = iteration(c4, key, N, P, step, kk, kp)
    return c4


def denoise_variance(accum, pass_count, guides, se, iterations, k_color, sigma_plane):
    """... from a Renderer.read_guides() dict and the error map's se (H x W)."""
    return denoise_variance4(rs.average(accum, pass_count), guides["key"], guides["normal"], guides["position"], se,
                             iterations, k_color, sigma_plane)


# ---- CPU checks
def test_binding_declares_variance_entry_points(mcpt_mod):
    L = mcpt_mod.lib()
    for name in ("mcpt_denoise_variance", "mcpt_denoise_resolved_variance", "mcpt_read_denoised_variance"):
        assert getattr(L, name).argtypes is not None, name
    for meth in ("denoise_variance", "denoise_resolved_variance", "read_denoised_variance"):
        assert callable(getattr(mcpt_mod.Renderer, meth))
    assert L.mcpt_denoise_variance(None, 1, 1.0, 1.0) == -1 and L.mcpt_denoise_resolved_variance(None, 1, 1.0, 1.0) == -1
    assert L.mcpt_read_denoised_variance(None, None) == -1
    assert mcpt_mod.DENOISE_K_VARIANCE > 0 and L.mcpt_version() == 2


def test_never_mixes_across_a_key_edge():
    """Colour and variance: side 1 holds colours in [5, 9] and se^2 in [100, 400], side 0 colours in
    [0, 1] and se^2 in [1e-4, 4e-4]; every output is a (near-)convex combination of its own side."""
    rng = np.random.default_rng(5)
    c, key, N, P, side = rs._two_sided(rng)
    se = np.where(side, rng.uniform(10, 20, key.shape), rng.uniform(0.01, 0.02, key.shape)).astype(np.float32)
    c0 = variance_init(c, key, se)
    assert np.array_equal(bits(c0[..., :3]), bits(c))
    for m in (side, ~side):
        lo, hi = (se[m] ** 2).min(), (se[m] ** 2).max()
        assert c0[..., 3][m].min() >= lo * F(1 - 1e-5) and c0[..., 3][m].max() <= hi * F(1 + 1e-5)
    out = denoise_variance4(c, key, N, P, se, 5, 4.0, 0.5)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    for m in (side, ~side):
        lo, hi = c[m].min(), c[m].max()
        assert out[..., :3][m].min() >= lo * F(1 - 1e-5) and out[..., :3][m].max() <= hi * F(1 + 1e-5)
    # the variance of a weighted mean (weights w / wsum, summing to 1) is at most the largest input
    # variance and, with at most 25 taps, at least 1/25 of the smallest: after two iterations side 1
    # holds at least 100 / 625, six decades above anything side 0 can hold
    two = denoise_variance4(c, key, N, P, se, 2, 4.0, 0.5)[..., 3]
    assert two[side].min() >= 100.0 / 625.0 * (1 - 1e-5) and two[~side].max() <= 4e-4 * (1 + 1e-5)
    assert out[..., 3][side].max() <= 400 * F(1 + 1e-5) and out[..., 3][~side].max() <= 4e-4 * (1 + 1e-5)
    # and it does filter where the variance says the spread is noise (side 1: sd 10..20 against colours
    # 4 apart), and does not where it says the spread is signal (side 0: sd 0.01..0.02 against 1)
    assert out[..., :3][side].std() < 0.5 * c[side].std()
    assert np.median(out[..., 3][side]) < 0.1 * np.median(c0[..., 3][side])
    assert out[..., :3][~side].std() > 0.9 * c[~side].std()


def _flat(Hh, Ww):
    key = np.full((Hh, Ww), (1 << 28) | 3, np.int32)
    N = np.zeros((Hh, Ww, 3), np.float32)
    N[...] = (0, 0, 1)
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    P = np.zeros((Hh, Ww, 3), np.float32)
    P[..., 0], P[..., 1] = xx, yy                     # a plane perpendicular to N: the plane term is 0
    return key, N, P


def test_flat_field_constant_variance():
    """The init step returns v exactly; one iteration returns v * sum(w^2) / sum(w)^2 over the in-frame
    taps (w = h[dy] h[dx]: colour, plane and normal terms are all 1)."""
    Hh, Ww = 9, 11
    key, N, P = _flat(Hh, Ww)
    c = np.full((Hh, Ww, 3), 0.625, np.float32)
    se = np.full((Hh, Ww), 0.375, np.float32)
    v = F(0.375) * F(0.375)                           # 9/64: gw * v and their sums are exact
    c0 = variance_init(c, key, se)
    assert np.array_equal(bits(c0[..., 3]), bits(np.full((Hh, Ww), v, np.float32)))
    se2 = np.full((Hh, Ww), 0.0123, np.float32)       # any v: within an ulp of the rounding of sv / sg
    v2 = F(0.0123) * F(0.0123)
    assert np.abs(variance_init(c, key, se2)[..., 3] - v2).max() <= np.spacing(v2)
    for step in (1, 2, 4):
        out = iteration(c0, key, N, P, step, F(16.0), F(1.0))
        assert np.abs(out[..., :3] - F(0.625)).max() <= np.spacing(F(0.625))
        h = H5.astype(np.float64)
        for y in range(Hh):
            for x in range(Ww):
                wy = np.array([h[d + 2] if 0 <= y + step * d < Hh else 0.0 for d in range(-2, 3)])
                wx = np.array([h[d + 2] if 0 <= x + step * d < Ww else 0.0 for d in range(-2, 3)])
                w = np.outer(wy, wx)
                want = float(v) * (w ** 2).sum() / w.sum() ** 2
                # 25 binary32 additions and a division: a few 2^-24 relative
                assert abs(float(out[y, x, 3]) - want) <= 32 * 2.0 ** -24 * want, (step, y, x)
    # the interior at step 1: (sum h^2)^2 / 1 = (35/128)^2
    out = iteration(c0, key, N, P, 1, F(16.0), F(1.0))
    assert abs(float(out[4, 5, 3]) / float(v) - (35.0 / 128.0) ** 2) < 1e-6


def test_zero_infinite_and_nan_standard_errors():
    """se of 0, +inf and NaN at single pixels: every output stays finite, the affected centres'
    variance is at most VMAX, and a NaN / inf neighbour raises a pixel's variance, never poisons it."""
    rng = np.random.default_rng(9)
    c, key, N, P, side = rs._two_sided(rng, 19, 23)
    se = rng.uniform(0.01, 0.1, key.shape).astype(np.float32)
    spots = {(3, 4): 0.0, (9, 12): np.inf, (15, 6): np.nan, (0, 0): np.nan, (18, 22): np.inf}
    for (y, x), val in spots.items():
        se[y, x] = val
    for it in (0, 1, 3, 5):
        out = denoise_variance4(c, key, N, P, se, it, 4.0, 0.75)
        assert np.isfinite(out).all(), it
        assert (out[..., 3] >= 0).all() and (out[..., 3] <= VMAX).all()
    c0 = variance_init(c, key, se)
    for (y, x), val in spots.items():
        assert c0[y, x, 3] <= VMAX
        if val != 0.0:
            assert c0[y, x, 3] >= VMAX * F(0.25)               # its own weight 1/4 of sg <= 1
    # a pixel all of whose 3x3 neighbours have se = 0 keeps variance 0 and kc = 2^40
    se0 = np.zeros(key.shape, np.float32)
    assert not variance_init(c, key, se0)[..., 3].any()


def test_zero_iterations_returns_c0():
    rng = np.random.default_rng(6)
    c, key, N, P, _ = rs._two_sided(rng, 9, 7)
    se = rng.uniform(0, 1, key.shape).astype(np.float32)
    acc = (c * F(3)).astype(np.float32)
    g = {"key": key, "normal": N, "position": P}
    out = denoise_variance(acc, 3, g, se, 0, 4.0, 1.0)
    assert np.array_equal(bits(out[..., :3]), bits(acc / F(3)))
    assert np.array_equal(bits(out), bits(variance_init(rs.average(acc, 3), key, se)))
    # with every variance 0 the filter is §3.8's guided one at se = 0 (kc = 2^40), bit for bit
    import test_stats_restate as st
    z = np.zeros(key.shape, np.float32)
    a = denoise_variance(acc, 3, g, z, 2, 4.0, 1.0)[..., :3]
    b = st.denoise_guided(acc, 3, g, z, 2, 4.0, 1.0)
    assert np.array_equal(bits(a), bits(b))
