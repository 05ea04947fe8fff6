"""The noise statistics' arithmetic contract, restated in numpy float32:
elementwise operations in the contract's order, nothing fused, so that tests/test_gpu_stats.py
can pin the HIP kernels bit for bit.  CPU checks of the restatement itself (the estimator against
synthetic samples of known variance, the corner cases) and of the binding's new entry points."""
import numpy as np

import test_denoise_restate as rs

F = np.float32
H5 = rs.H5
bits = rs.bits
R_MAX = F(64.0)
Q_SCALE = F(65536.0)


def luminance(accum):
    """Y of accumulator pixels (.., 3): (0.2126 R + 0.7152 G) + 0.0722 B on the sums."""
    a = np.asarray(accum, np.float32)
    with np.errstate(all="ignore"):
        y = (F(0.2126) * a[..., 0] + F(0.7152) * a[..., 1]) + F(0.0722) * a[..., 2]
    assert y.dtype == np.float32
    return y


def begin(accum):
    """A window's state: Yacc = Ybase = Y(accum), S2 = 0, N = B = 0."""
    y = luminance(accum)
    return {"Yacc": y.copy(), "S2": np.zeros_like(y), "Ybase": y.copy(), "N": 0, "B": 0}


def batch(st, accum, n):
    """The accumulator now holds n more passes than at the previous batch (updates st in place)."""
    assert n > 0
    with np.errstate(all="ignore"):
        ynow = luminance(accum)
        d = ynow - st["Yacc"]
        st["S2"] = (st["S2"] + (d * d) / F(n)).astype(np.float32)
    st["Yacc"] = ynow
    st["N"] += int(n)
    st["B"] += 1
    return st


def error(st, mu_floor):
    """(se, r, q) per pixel; needs B >= 2."""
    assert st["B"] >= 2
    nf, bm1 = F(st["N"]), F(st["B"] - 1)
    with np.errstate(all="ignore"):
        s1 = st["Yacc"] - st["Ybase"]
        v = st["S2"] - (s1 * s1) / nf
        v = np.where(F(0) < v, v, F(0)).astype(np.float32)         # (a NaN v gives 0)
        var = v / bm1
        se = np.sqrt(var / nf)
        mu = s1 / nf
        r = se / (np.where(F(0) < mu, mu, F(0)).astype(np.float32) + F(mu_floor))
        bad = ~np.isfinite(st["S2"]) | ~np.isfinite(s1) | ~(r <= R_MAX)
        r = np.where(bad, R_MAX, r).astype(np.float32)
        q = (r * Q_SCALE).astype(np.uint32)                          # truncation; r in [0, 64]
    assert se.dtype == np.float32 and r.dtype == np.float32
    return se, r, q


def record(r, q, threshold):
    """The frame record of the pixels given (any shape)."""
    n_px = int(r.size)
    sum_q = int(q.astype(np.uint64).sum())
    max_r = F(r.max()) if n_px else F(0)
    return {"n_px": n_px, "n_above": int((r > F(threshold)).sum()), "sum_q": sum_q, "max_r": max_r,
            "mean_r": (sum_q / 65536.0 / n_px) if n_px else 0.0}


def add_records(a, b):
    """The record of two disjoint sets of pixels from their records."""
    n = a["n_px"] + b["n_px"]
    s = a["sum_q"] + b["sum_q"]
    return {"n_px": n, "n_above": a["n_above"] + b["n_above"], "sum_q": s, "max_r": max(a["max_r"], b["max_r"]),
            "mean_r": s / 65536.0 / n}


def guided_constants(s, k_color, sigma_plane):
    """(step, k_color * 2^-s, kp[s]) in binary32, as the host computes them."""
    step, _, kp = rs.constants(s, 1.0, sigma_plane)
    return step, F(F(k_color) * F(2.0 ** -s)), kp


def guided_kc(ks, se):
    """kc per centre pixel: sg = ks * se; kc = 1 / (sg * sg + 2^-40)."""
    with np.errstate(all="ignore"):
        sg = (F(ks) * np.asarray(se, np.float32)).astype(np.float32)
        return (F(1) / (sg * sg + F(2.0 ** -40))).astype(np.float32)


def iteration_kc_map(c, key, N, P, step, kc, kp):
    """§3.7's iteration (test_denoise_restate.iteration, operation for operation) with kc an H x W
    array taken at the centre pixel."""
    c = np.asarray(c, np.float32)
    Hh, Ww = key.shape
    h22 = F(H5[2] * H5[2])
    acc = (h22 * c).astype(np.float32)
    wsum = np.full((Hh, Ww), h22, np.float32)
    with np.errstate(all="ignore"):
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
        return (acc / wsum[..., None]).astype(np.float32)


def denoise_guided(accum, pass_count, guides, se, iterations, k_color, sigma_plane):
    """The guided filter from a Renderer.read_guides() dict and the error map's se (H x W); se is
    not refiltered between the iterations."""
    c = rs.average(accum, pass_count)
    for s in range(iterations):
        step, ks, kp = guided_constants(s, k_color, sigma_plane)
        c = iteration_kc_map(c, guides["key"], guides["normal"], guides["position"], step, guided_kc(ks, se), kp)
    return c


# ---- CPU checks
def _gray(y):
    """Accumulator pixels whose three channels are y."""
    y = np.asarray(y, np.float32)
    return np.repeat(y[..., None], 3, axis=-1)


def _run_window(samples, sizes):
    """samples: passes x pixels per-pass values (float64); batches of the given sizes."""
    cum = np.concatenate([np.zeros((1, samples.shape[1])), np.cumsum(samples, axis=0)])
    st = begin(_gray(cum[0]))
    at = 0
    for n in sizes:
        at += n
        batch(st, _gray(cum[at]), n)
    assert at == samples.shape[0]
    return st


def _variance_estimate(st):
    s1 = st["Yacc"] - st["Ybase"]
    v = st["S2"] - (s1 * s1) / F(st["N"])
    return v / F(st["B"] - 1)


def _check_estimator(sizes, seed):
    """Per-pass luminances x ~ Normal(mu, sigma^2), i.i.d.  The batch means m_b are then
    Normal(mu, sigma^2 / n_b), so Q = sum n_b (m_b - m)^2 / sigma^2 (m the weighted mean) is exactly
    chi-square with B - 1 degrees of freedom for ANY batch sizes, and the estimate v / (B - 1) =
    sigma^2 Q / (B - 1) has mean sigma^2 and relative standard deviation sqrt(2 / (B - 1)).
    Bounds: every pixel within 5 of those standard deviations (for B - 1 >= 63 the chi-square's
    skew moves the 5-sigma tails by less than a factor that matters at 256 pixels: P < 1e-5 per
    pixel), and the mean over the P independent pixels within 5 standard deviations of ITS spread,
    sqrt(2 / ((B - 1) P)).  Binary32 slack: S2 ~ N (mu^2 + sigma^2) is formed by B additions each
    within 2^-24 S2, the accumulators' rounding (2^-24 N mu per snapshot) reaches d^2 / n with
    factor 2 d / n ~ 2 mu: together below (2 B) 2^-24 N (mu^2 + sigma^2) / ((B - 1) sigma^2) ~ 1e-4
    relative for N <= 1024, mu = sigma = 0.5; 1e-3 is allowed."""
    mu, sigma, P = 0.5, 0.5, 256
    rng = np.random.default_rng(seed)
    x = rng.normal(mu, sigma, (int(sum(sizes)), P))
    st = _run_window(x, sizes)
    B = len(sizes)
    assert st["B"] == B >= 64 and st["N"] == sum(sizes)
    ratio = _variance_estimate(st).astype(np.float64) / sigma ** 2
    sd = np.sqrt(2.0 / (B - 1))
    assert np.abs(ratio - 1.0).max() <= 5 * sd + 1e-3, (ratio.min(), ratio.max(), sd)
    assert abs(ratio.mean() - 1.0) <= 5 * sd / np.sqrt(P) + 1e-3, (ratio.mean(), sd / np.sqrt(P))
    # the standard error of the window's mean is then sigma / sqrt(N), within the same spread
    se, r, _ = error(st, 0.01)
    want = sigma / np.sqrt(st["N"])
    assert np.abs(se.astype(np.float64) ** 2 / want ** 2 - 1.0).max() <= 5 * sd + 2e-3
    assert (r < 1).all()


def test_estimator_equal_batches():
    _check_estimator([8] * 64, seed=11)


def test_estimator_unequal_batches():
    _check_estimator([1, 2, 3, 5, 8, 13, 4, 32, 7, 21, 16] * 6, seed=12)      # B = 66, N = 672


def test_constant_pixel_has_zero_error():
    st = begin(_gray(np.zeros(5)))
    for n in (4, 4, 8, 3):
        batch(st, _gray(np.full(5, 0.0)), n)            # a pixel that no pass changes (black)
    se, r, q = error(st, 0.01)
    assert (bits(se) == 0).all() and (bits(r) == 0).all() and (q == 0).all()
    # ... and one that holds light from before the window and gains none in it
    st = begin(_gray(np.full(5, 37.25)))
    for n in (1, 1, 5):
        batch(st, _gray(np.full(5, 37.25)), n)
    se, r, q = error(st, 0.01)
    assert (bits(se) == 0).all() and (bits(r) == 0).all() and (q == 0).all()
    # a pixel that gains exactly 0.75 per pass: Y(0.75 n) is not exactly 0.75 n (the weights are not
    # dyadic), so the batch means agree only up to rounding; what is left is rounding noise, below
    # one part in 10^5 of the mean
    st = begin(_gray(np.zeros(3)))
    tot = 0
    for n in (4, 4, 8, 3, 1):
        tot += n
        batch(st, _gray(np.full(3, 0.75 * tot)), n)
    se, r, q = error(st, 0.01)
    assert (se <= F(1e-6)).all() and (r <= F(1e-5)).all(), (se, r)


def test_overflowed_pixel_counts_as_unconverged():
    acc0 = np.zeros((2, 3), np.float32)
    st = begin(acc0)
    acc1 = np.array([[1e30, 1e30, 1e30], [1.0, 2.0, 3.0]], np.float32)
    batch(st, acc1, 4)
    batch(st, acc1 + np.array([[0, 0, 0], [1.5, 1.0, 0.5]], np.float32), 4)
    assert np.isinf(st["S2"][0]) and np.isfinite(st["S2"][1])
    se, r, q = error(st, 0.01)
    assert r[0] == F(64) and int(q[0]) == 4194304
    assert np.isfinite(r[1]) and r[1] < 64 and int(q[1]) == int(np.floor(float(r[1]) * 65536.0))
    assert not np.isnan(se).any()
    # an accumulator that already holds 1e30 when the window begins, unchanged since: S2 stays 0,
    # but 1e30 - 1e30 = 0 is "no light at all": converged, not overflowed; NaN / inf sums are
    st = begin(np.array([[np.inf, 0, 0], [np.nan, 1, 1]], np.float32))
    batch(st, np.array([[np.inf, 0, 0], [np.nan, 1, 1]], np.float32), 2)
    batch(st, np.array([[np.inf, 0, 0], [np.nan, 1, 1]], np.float32), 2)
    se, r, q = error(st, 0.01)
    assert (r == F(64)).all() and (q == 4194304).all()


def test_record_of_disjoint_halves_adds_up():
    rng = np.random.default_rng(3)
    x = rng.gamma(0.7, 1.0, (40, 333))
    x[:, 17] = 0.0
    st = _run_window(x, [4, 4, 8, 3, 1, 20])
    se, r, q = error(st, 0.02)
    whole = record(r, q, 0.1)
    a, b = record(r[:100], q[:100], 0.1), record(r[100:], q[100:], 0.1)
    s = add_records(a, b)
    for k in ("n_px", "n_above", "sum_q"):
        assert s[k] == whole[k], k
    assert bits(s["max_r"]) == bits(whole["max_r"]) and s["mean_r"] == whole["mean_r"]
    assert 0 < whole["n_above"] < whole["n_px"] and whole["sum_q"] == int(q.astype(object).sum())
    assert abs(whole["mean_r"] - float(r.astype(np.float64).mean())) <= 2.0 ** -16


def test_guided_iteration_is_the_fixed_one_with_a_kc_map():
    """A constant kc map reproduces §3.7's iteration bit for bit (the two restatements cannot
    drift apart), se = 0 keeps only taps of equal colour, and the width follows se."""
    rng = np.random.default_rng(8)
    c, key, N, P, side = rs._two_sided(rng, 19, 23)
    for s in (0, 2):
        step, kc, kp = rs.constants(s, 1.5, 0.75)
        a = rs.iteration(c, key, N, P, step, kc, kp)
        b = iteration_kc_map(c, key, N, P, step, np.full(key.shape, kc, np.float32), kp)
        assert np.array_equal(bits(a), bits(b))
    g = {"key": key, "normal": N, "position": P}
    zero = denoise_guided(c * F(4), 4, g, np.zeros(key.shape, np.float32), 3, 4.0, 1.0)
    # kc = 2^40: a tap differing by 2^-12 or more in any channel weighs < 2^-30; the uniform(0, 1)
    # colours of this frame all differ by far more, so the image stays as it is to ~1e-6
    assert np.abs(zero - rs.average(c * F(4), 4)).max() < 1e-5
    flat = c.copy()
    flat[...] = 0.25
    out = denoise_guided(flat, 1, g, np.zeros(key.shape, np.float32), 3, 4.0, 1.0)
    assert np.abs(out - F(0.25)).max() <= np.spacing(F(0.25))      # equal colours: still averaged
    wide = denoise_guided(c, 1, g, np.full(key.shape, 1.0, np.float32), 4, 4.0, 1.0)
    narrow = denoise_guided(c, 1, g, np.full(key.shape, 0.01, np.float32), 4, 4.0, 1.0)
    assert wide[~side].std() < 0.5 * narrow[~side].std()
    assert np.array_equal(bits(guided_kc(F(0.5), np.array([0.0], np.float32))), bits(np.array([2.0 ** 40], np.float32)))


def test_binding_declares_stats_entry_points(mcpt_mod):
    L = mcpt_mod.lib()
    for name in ("mcpt_stats_begin", "mcpt_stats_end", "mcpt_stats_add_batch", "mcpt_stats_info", "mcpt_convergence",
                 "mcpt_read_error_map", "mcpt_denoise_guided", "mcpt_last_stats_ms"):
        assert getattr(L, name).argtypes is not None, name
    for meth in ("stats_begin", "stats_end", "stats_add_batch", "stats_info", "convergence", "read_error_map",
                 "denoise_guided", "render_until", "last_stats_ms"):
        assert callable(getattr(mcpt_mod.Renderer, meth))
    assert b"statistics" in L.mcpt_error_string(-8)
    assert L.mcpt_convergence(None, 1.0, 1.0, None) == -1 and L.mcpt_stats_begin(None) == -1
    assert L.mcpt_denoise_guided(None, 1, 1.0, 1.0) == -1 and L.mcpt_version() == 2
    assert mcpt_mod.DENOISE_K_COLOR > 0 and mcpt_mod.ERROR_MU_FLOOR > 0
