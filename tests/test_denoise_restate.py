"""The à-trous denoiser's arithmetic contract, restated in numpy float32:
elementwise operations in the contract's order (no np.dot / einsum, nothing fused), so that
tests/test_gpu_denoise.py can pin the HIP kernels bit for bit.  CPU checks of the restatement
itself, and of the binding's new entry points."""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)


def average(accum, pass_count):
    """Iteration 0's input: accum / pass_count, one binary32 division per channel."""
    return (np.asarray(accum, np.float32) / F(pass_count)).astype(np.float32)


def constants(s, sigma_color, sigma_plane):
    """(step, kc[s], kp[s]) in binary32, as the host computes them."""
    step = 1 << s
    sc = F(F(sigma_color) * F(2.0 ** -s))
    sp = F(F(sigma_plane) * F(step))
    return step, F(F(1) / F(sc * sc)), F(F(1) / F(sp * sp))


def iteration(c, key, N, P, step, kc, kp):
    """One iteration: c, N, P are H x W x 3 float32, key H x W int32."""
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
                    continue                      # every tap outside the frame
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                kp_, kq_ = key[p], key[q]
                ok = kq_ == kp_
                cp, cq, Np, Nq, Pp, Pq = c[p], c[q], N[p], N[q], P[p], P[q]
                dc = cq - cp
                a_c = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * kc
                dP = Pq - Pp
                t = (Np[..., 0] * dP[..., 0] + Np[..., 1] * dP[..., 1]) + Np[..., 2] * dP[..., 2]
                a_p = (t * t) * kp
                d = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                nd = np.where(F(0) < d, d, F(0)).astype(np.float32)      # max(0, d), GLSL definition
                for _ in range(5):
                    nd = nd * nd
                wn = np.where(kp_ < 0, F(1), nd).astype(np.float32)
                r = F(1) / (F(1) + (a_c + a_p))
                w = (((F(H5[dy + 2] * H5[dx + 2])) * wn) * r) * r
                assert w.dtype == np.float32 and a_c.dtype == np.float32 and a_p.dtype == np.float32
                acc[p] = np.where(ok[..., None], acc[p] + w[..., None] * cq, acc[p])
                wsum[p] = np.where(ok, wsum[p] + w, wsum[p])
        return (acc / wsum[..., None]).astype(np.float32)


def denoise(accum, pass_count, key, N, P, iterations, sigma_color, sigma_plane):
    c = average(accum, pass_count)
    for s in range(iterations):
        step, kc, kp = constants(s, sigma_color, sigma_plane)
        c = iteration(c, key, N, P, step, kc, kp)
    return c


def denoise_guides(accum, pass_count, guides, iterations, sigma_color, sigma_plane):
    """... from a Renderer.read_guides() dict."""
    return denoise(accum, pass_count, guides["key"], guides["normal"], guides["position"], iterations, sigma_color,
                   sigma_plane)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- CPU checks
def _two_sided(rng, Hh=23, Ww=31):
    """A frame cut by a slanted key edge: side 0 (key 1 << 28 | 3) holds values in [0, 1], side 1
    (a miss, key -1) values in [5, 9]; smooth guides on each side."""
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    side = (xx + yy // 2) > Ww // 2
    key = np.where(side, -1, (1 << 28) | 3).astype(np.int32)
    c = np.where(side[..., None], rng.uniform(5, 9, (Hh, Ww, 3)), rng.uniform(0, 1, (Hh, Ww, 3))).astype(np.float32)
    N = np.zeros((Hh, Ww, 3), np.float32)
    N[~side] = (0, 0, 1)
    P = np.zeros((Hh, Ww, 3), np.float32)
    P[..., 0], P[..., 1] = xx, yy
    P[side] = 0
    return c, key, N, P, side


def test_restatement_never_mixes_across_a_key_edge():
    rng = np.random.default_rng(5)
    c, key, N, P, side = _two_sided(rng)
    out = denoise(c * F(4), 4, key, N, P, 5, 16.0, 0.5)
    assert out.dtype == np.float32 and np.isfinite(out).all()
    for m in (side, ~side):
        lo, hi = c[m].min(), c[m].max()
        # a convex combination of one side's inputs, up to the rounding of sum / wsum
        assert out[m].min() >= lo * F(1 - 1e-5) and out[m].max() <= hi * F(1 + 1e-5)
    assert out[side].min() > 4 and out[~side].max() < 2
    # and it does filter: the spread inside each side shrinks
    assert out[side].std() < 0.5 * c[side].std() and out[~side].std() < 0.5 * c[~side].std()


def test_restatement_fixed_points():
    rng = np.random.default_rng(6)
    c, key, N, P, _ = _two_sided(rng, 9, 7)
    acc = (c * F(3)).astype(np.float32)
    assert np.array_equal(bits(denoise(acc, 3, key, N, P, 0, 1.0, 1.0)), bits(acc / F(3)))
    # a constant image is a fixed point wherever sum / wsum is exact; within an ulp elsewhere
    flat = np.full_like(c, 0.625)
    out = denoise(flat, 1, key, N, P, 4, 1.0, 1.0)
    assert np.abs(out - F(0.625)).max() <= np.spacing(F(0.625))
    # an overflowing colour distance gives weight 0, not NaN
    big = c.copy()
    big[4, 3] = 1e30
    out = denoise(big, 1, np.full_like(key, 7), N, P, 3, 1.0, 1.0)
    assert np.isfinite(out).all()


def test_binding_declares_denoise_entry_points(mcpt_mod):
    L = mcpt_mod.lib()
    for name in ("mcpt_render_guides", "mcpt_read_guides", "mcpt_denoise", "mcpt_read_denoised",
                 "mcpt_last_denoise_ms"):
        assert getattr(L, name).argtypes is not None, name
    for meth in ("render_guides", "read_guides", "denoise", "last_denoise_ms"):
        assert callable(getattr(mcpt_mod.Renderer, meth))
    assert L.mcpt_error_string(-7) and b"guide" in L.mcpt_error_string(-7)
    assert L.mcpt_denoise(None, 1, 1.0, 1.0) == -1 and L.mcpt_render_guides(None, None, None) == -1
