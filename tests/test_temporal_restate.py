"""Temporal reprojection's arithmetic contract, restated in numpy float32:
elementwise operations in the contract's order, nothing fused, so that tests/test_gpu_temporal.py can
pin the HIP kernel bit for bit.  CPU checks of the restatement itself, of mat4_inverse and of the
binding's argument checks."""
import os
import sys

import numpy as np
import pytest

import test_variance_restate as vr

F = np.float32
VMAX = vr.VMAX
bits = vr.bits
G3 = vr.G3
FLT_MAX = np.finfo(np.float32).max
KEYS = ("n_px", "n_history", "n_new", "n_miss", "n_offscreen", "n_rejected", "sum_len", "max_len")


def current(accum, pass_count, se):
    """{c, v} H x W x 4: accum / (float)pass_count and min(se^2, 2^60) (NaN and inf: 2^60)."""
    with np.errstate(all="ignore"):
        c = (np.asarray(accum, np.float32) / F(pass_count)).astype(np.float32)
        t = (np.asarray(se, np.float32) * np.asarray(se, np.float32)).astype(np.float32)
        v = np.where(t < VMAX, t, VMAX).astype(np.float32)
    return np.concatenate([c, v[..., None]], axis=-1).astype(np.float32)


def accumulate(cv, guides, hist, prevPV, max_history, plane_tol):
    """One accumulate.  cv: current(); guides: a Renderer.read_guides() dict of the current frame;
    hist: None (empty) or the dict a previous call returned; prevPV: 16 floats, column-major.
    Returns (the new history {"c": H x W x 4, "len": H x W i32, "key", "normal", "position"}, the
    record's dict)."""
    cv = np.asarray(cv, np.float32)
    key, N, P, dist = guides["key"], guides["normal"], guides["position"], guides["dist"]
    Hh, Ww = key.shape
    miss = key < 0
    out = cv.copy()
    length = np.ones((Hh, Ww), np.int32)
    has = np.zeros((Hh, Ww), bool)
    inb = np.zeros((Hh, Ww), bool)
    if hist is not None:
        M = np.asarray(prevPV, np.float32).reshape(16)
        hc, hl, hk, hN, hP = hist["c"], hist["len"], hist["key"], hist["normal"], hist["position"]
        with np.errstate(all="ignore"):
            Px, Py, Pz = P[..., 0], P[..., 1], P[..., 2]
            w = ((M[3] * Px + M[7] * Py) + M[11] * Pz) + M[15]
            cx = ((M[0] * Px + M[4] * Py) + M[8] * Pz) + M[12]
            cy = ((M[1] * Px + M[5] * Py) + M[9] * Pz) + M[13]
            iw = F(1) / w
            sx = ((cx * iw) * F(0.5) + F(0.5)) * F(Ww) - F(0.5)
            sy = ((cy * iw) * F(0.5) + F(0.5)) * F(Hh) - F(0.5)
            assert w.dtype == sx.dtype == sy.dtype == np.float32
            inb = ~miss & (F(0) < w) & (F(-1) < sx) & (sx < F(Ww)) & (F(-1) < sy) & (sy < F(Hh))
            flx = np.where(inb, np.floor(sx), F(0)).astype(np.float32)
            fly = np.where(inb, np.floor(sy), F(0)).astype(np.float32)
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            fx, fy = (sx - flx).astype(np.float32), (sy - fly).astype(np.float32)
            tol = F(plane_tol) * dist
            tol2 = tol * tol
            bs = np.zeros((Hh, Ww), np.float32)
            acc = np.zeros((Hh, Ww, 4), np.float32)
            lmin = np.full((Hh, Ww), 65535, np.int32)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    ok = inb & (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                    qxc, qyc = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                    ok &= hk[qyc, qxc] == key
                    dP = hP[qyc, qxc] - P
                    t = (N[..., 0] * dP[..., 0] + N[..., 1] * dP[..., 1]) + N[..., 2] * dP[..., 2]
                    ok &= t * t <= tol2
                    Nq = hN[qyc, qxc]
                    nd = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    ok &= F(0.875) <= nd
                    b = ((fx if i else F(1) - fx) * (fy if j else F(1) - fy)).astype(np.float32)
                    assert b.dtype == t.dtype == nd.dtype == np.float32
                    acc = np.where(ok[..., None], acc + b[..., None] * hc[qyc, qxc], acc).astype(np.float32)
                    bs = np.where(ok, bs + b, bs).astype(np.float32)
                    lmin = np.where(ok, np.minimum(lmin, hl[qyc, qxc]), lmin).astype(np.int32)
            has = inb & (F(0) < bs)
            h = (acc / bs[..., None]).astype(np.float32)
            L = np.minimum(lmin + 1, max_history).astype(np.int32)
            a = (F(1) / L.astype(np.float32)).astype(np.float32)
            k = (F(1) - a).astype(np.float32)
            blend = np.empty_like(cv)
            blend[..., :3] = k[..., None] * h[..., :3] + a[..., None] * cv[..., :3]
            blend[..., 3] = (k * k) * h[..., 3] + (a * a) * cv[..., 3]
        out = np.where(has[..., None], blend, cv).astype(np.float32)
        length = np.where(has, L, 1).astype(np.int32)
    n_off = int((~miss & ~inb).sum()) if hist is not None else 0
    n_rej = int((~miss & ~has).sum()) - n_off
    rec = {"n_px": Hh * Ww, "n_history": int(has.sum()), "n_miss": int(miss.sum()), "n_offscreen": n_off,
           "n_rejected": n_rej, "sum_len": int(length.sum()), "max_len": int(length.max())}
    rec["n_new"] = rec["n_miss"] + rec["n_offscreen"] + rec["n_rejected"]
    new = {"c": out, "len": length, "key": key.copy(), "normal": N.copy(), "position": P.copy()}
    return new, rec


def prefilter(c4, key):
    """The variance filter's first input from the temporal image: {rgb, the 3x3 key-aware prefilter of
    its variance} (vr.variance_init's taps, weights and order, on v itself)."""
    c4 = np.asarray(c4, np.float32)
    Hh, Ww = key.shape
    v = c4[..., 3]
    with np.errstate(all="ignore"):
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
                sv[p] = np.where(ok, sv[p] + gw * v[q], sv[p])
                sg[p] = np.where(ok, sg[p] + gw, sg[p])
        out = c4.copy()
        out[..., 3] = sv / sg
    return out


def denoise_temporal(c4, guides, iterations, k_color, sigma_plane):
    """H x W x 4 {rgb, variance}: the variance filter's iterations from prefilter(c4)."""
    key, N, P = guides["key"], guides["normal"], guides["position"]
    x = prefilter(c4, key)
    kk = F(F(k_color) * F(k_color))
    for s in range(iterations):
        step, _, kp = vr.rs.constants(s, 1.0, sigma_plane)
        x = vr.iteration(x, key, N, P, step, kk, kp)
    return x


# ---- cameras (what the tests and tools move)
def orbit_camera(mcpt, W, H, deg):
    """(invPV, invV, PV) of the canonical camera with the world turned `deg` degrees about its up
    axis (z): PV' = PV R, so invPV' = R^-1 invPV and invV' = R^-1 invV."""
    ipv, iv = mcpt.camera_canonical(W, H)
    rinv = mcpt.Transfo.rotateZ(-deg)
    ipv2, iv2 = mcpt.Transfo.mul(rinv, ipv), mcpt.Transfo.mul(rinv, iv)
    return ipv2, iv2, mcpt.mat4_inverse(ipv2)


def turned_pv(mcpt, invPV, invV, deg):
    """P·V of the camera (invPV, invV) turned `deg` degrees about its own y axis: P Ry V."""
    pv, v = mcpt.mat4_inverse(invPV), mcpt.mat4_inverse(invV)
    p = mcpt.Transfo.mul(pv, invV)
    return mcpt.Transfo.mul(p, mcpt.Transfo.rotateY(deg), v)


def plane_guides(mcpt, W, H, invPV, invV, z=0.0):
    """Guides of the plane z = const under a camera: N = (0, 0, 1), one key; rays that leave the plane
    behind are misses."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden as g
    key = np.full((H, W), -1, np.int32)
    N = np.zeros((H, W, 3), np.float32)
    P = np.zeros((H, W, 3), np.float32)
    dist = np.full((H, W), FLT_MAX, np.float32)
    for y in range(H):
        for x in range(W):
            o, d, _, _ = g.camera_dir(invPV, invV, W, H, x, y)
            o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
            if d[2] == 0:
                continue
            t = (z - o[2]) / d[2]
            if t > 0:
                key[y, x], N[y, x], P[y, x], dist[y, x] = (4 << 28) | 7, (0, 0, 1), o + t * d, t
    return {"key": key, "normal": N, "position": P, "dist": dist}


@pytest.fixture(scope="module")
def plane(mcpt_mod):
    W, H = 16, 12
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    g = plane_guides(mcpt_mod, W, H, ipv, iv)
    assert (g["key"] >= 0).sum() > W * H // 2
    return W, H, ipv, iv, g


def _frame(rng, W, H, passes=4):
    acc = rng.uniform(0, 4, (H, W, 3)).astype(np.float32)
    se = rng.uniform(0.01, 0.2, (H, W)).astype(np.float32)
    return current(acc, passes, se), acc, se


# ---- CPU checks
def test_empty_history_starts_every_pixel(plane):
    W, H, ipv, iv, g = plane
    cv, acc, se = _frame(np.random.default_rng(1), W, H)
    hist, rec = accumulate(cv, g, None, None, 8, 0.01)
    assert np.array_equal(bits(hist["c"]), bits(cv)) and (hist["len"] == 1).all()
    assert np.array_equal(bits(cv[..., :3]), bits(acc / F(4))) and np.array_equal(bits(cv[..., 3]), bits(se * se))
    n_miss = int((g["key"] < 0).sum())
    assert rec == {"n_px": W * H, "n_history": 0, "n_new": W * H, "n_miss": n_miss, "n_offscreen": 0,
                   "n_rejected": W * H - n_miss, "sum_len": W * H, "max_len": 1}
    # the first frame's filter input is the variance filter's own (vr.variance_init), bit for bit
    assert np.array_equal(bits(prefilter(hist["c"], g["key"])), bits(vr.variance_init(cv[..., :3], g["key"], se)))


def test_same_camera_counts_up_to_the_cap(mcpt_mod, plane):
    W, H, ipv, iv, g = plane
    pv = mcpt_mod.mat4_inverse(ipv)
    rng = np.random.default_rng(2)
    hit = g["key"] >= 0
    hist = None
    for k in range(1, 7):
        cv, _, _ = _frame(rng, W, H)
        hist, rec = accumulate(cv, g, hist, pv, 4, 0.01)
        want = min(k, 4)
        assert (hist["len"][hit] == want).all() and (hist["len"][~hit] == 1).all(), k
        assert rec["n_history"] == (int(hit.sum()) if k > 1 else 0) and rec["max_len"] == want
        assert rec["n_offscreen"] == 0 and rec["n_rejected"] == (0 if k > 1 else int(hit.sum()))
        assert rec["n_new"] == rec["n_px"] - rec["n_history"]
        assert np.array_equal(bits(hist["c"][~hit]), bits(cv[~hit]))


def test_constant_history_and_frame_stay_constant(mcpt_mod, plane):
    """c = 0.5 and v = 2^-6 everywhere: b * 0.5 is exact, so sum = 0.5 * bs and h = 0.5 exactly; the
    blend k * 0.5 + a * 0.5 rounds k + a once: within one ulp of 0.5.  The variance is
    (k^2 + a^2) * 2^-6 <= 2^-6."""
    W, H, ipv, iv, g = plane
    pv = mcpt_mod.mat4_inverse(ipv)
    cv = np.zeros((H, W, 4), np.float32)
    cv[..., :3], cv[..., 3] = 0.5, 2.0 ** -6
    hist = None
    for k in range(1, 6):
        hist, _ = accumulate(cv, g, hist, pv, 32, 0.01)
        assert np.abs(hist["c"][..., :3] - F(0.5)).max() <= np.spacing(F(0.5)), k
        assert (hist["c"][..., 3] <= F(2.0 ** -6)).all()
    hit = g["key"] >= 0
    # five equal frames: the variance of the mean is near v / 5
    assert np.abs(hist["c"][..., 3][hit] * 5 / 2.0 ** -6 - 1).max() < 1e-5


def test_camera_turned_around_is_offscreen(mcpt_mod, plane):
    W, H, ipv, iv, g = plane
    rng = np.random.default_rng(3)
    cv, _, _ = _frame(rng, W, H)
    hist, _ = accumulate(cv, g, None, None, 8, 0.01)
    cv2, _, _ = _frame(rng, W, H)
    back = turned_pv(mcpt_mod, ipv, iv, 180.0)
    hist2, rec = accumulate(cv2, g, hist, back, 8, 0.01)
    n_miss = int((g["key"] < 0).sum())
    assert rec["n_offscreen"] == W * H - n_miss and rec["n_history"] == 0 and rec["n_rejected"] == 0
    assert np.array_equal(bits(hist2["c"]), bits(cv2)) and (hist2["len"] == 1).all()


def test_nan_and_inf_take_the_contracts_paths(mcpt_mod, plane):
    W, H, ipv, iv, g = plane
    pv = mcpt_mod.mat4_inverse(ipv)
    rng = np.random.default_rng(4)
    hit = np.argwhere(g["key"] >= 0)
    (ya, xa), (yb, xb), (yc, xc) = hit[len(hit) // 2], hit[len(hit) // 3], hit[2 * len(hit) // 3]
    _, acc, se = _frame(rng, W, H)
    se[ya, xa], se[yb, xb] = np.nan, np.inf
    acc[yc, xc] = (1e30 * 4, np.inf, 1.0)
    cv = current(acc, 4, se)
    assert cv[ya, xa, 3] == VMAX and cv[yb, xb, 3] == VMAX and np.isinf(cv[yc, xc, 1])
    hist, _ = accumulate(cv, g, None, None, 8, 0.01)
    cv2, _, _ = _frame(rng, W, H)
    hist2, rec = accumulate(cv2, g, hist, pv, 8, 0.01)
    assert rec["n_history"] == len(hit)
    assert np.isfinite(hist2["c"][..., 3]).all() and hist2["c"][ya, xa, 3] >= VMAX / 8
    assert not np.isfinite(hist2["c"][yc, xc, 1]) and hist2["c"][yc, xc, 0] >= 1e29     # propagates as written
    # a NaN position fails the bounds test: offscreen, not a fault
    g2 = {k: v.copy() for k, v in g.items()}
    g2["position"][ya, xa] = np.nan
    _, rec2 = accumulate(cv2, g2, hist, pv, 8, 0.01)
    assert rec2["n_offscreen"] == 1 and rec2["n_history"] == len(hit) - 1


def test_max_history_one_never_blends(mcpt_mod, plane):
    W, H, ipv, iv, g = plane
    pv = mcpt_mod.mat4_inverse(ipv)
    rng = np.random.default_rng(5)
    hist = None
    for _ in range(3):
        cv, _, _ = _frame(rng, W, H)
        hist, rec = accumulate(cv, g, hist, pv, 1, 0.01)
        assert np.array_equal(bits(hist["c"]), bits(cv)) and rec["max_len"] == 1      # k = 0, a = 1


def test_mat4_inverse_against_numpy(mcpt_mod):
    rng = np.random.default_rng(6)
    for _ in range(20):
        a = rng.normal(size=(4, 4)).astype(np.float32)
        got = mcpt_mod.mat4_inverse(a.T.reshape(-1)).reshape(4, 4).T
        want = np.linalg.inv(a.astype(np.float64))
        # double arithmetic rounded once: the conditioning times 2^-53, plus the rounding to binary32
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max() * 2
    ipv, _ = mcpt_mod.camera_canonical(37, 21)
    pv = mcpt_mod.mat4_inverse(ipv).reshape(4, 4).T.astype(np.float64)
    assert np.abs(pv @ ipv.reshape(4, 4).T.astype(np.float64) - np.eye(4)).max() < 1e-5
    L = mcpt_mod.lib()
    out = np.full(16, 7.0, np.float32)
    dup = np.arange(16, dtype=np.float32).reshape(4, 4)
    dup[2] = dup[1]
    for bad in (np.zeros(16, np.float32), dup.reshape(-1), np.full(16, np.nan, np.float32)):
        bad = np.ascontiguousarray(bad, np.float32)
        assert L.mcpt_mat4_inverse(mcpt_mod._fp(bad), mcpt_mod._fp(out)) == -1
        assert (out == 7.0).all()
        with pytest.raises(mcpt_mod.MCPTError):
            mcpt_mod.mat4_inverse(bad)
    assert L.mcpt_mat4_inverse(None, mcpt_mod._fp(out)) == -1 and L.mcpt_mat4_inverse(mcpt_mod._fp(out), None) == -1


def test_binding_argument_checks_need_no_device(mcpt_mod):
    L = mcpt_mod.lib()
    rec = mcpt_mod.TemporalRecord()
    assert L.mcpt_temporal_begin(None) == -1 and L.mcpt_temporal_end(None) == -1
    assert L.mcpt_temporal_accumulate(None, None, 8, 0.01, rec) == -1
    assert L.mcpt_denoise_temporal(None, 1, 1.0, 1.0) == -1 and L.mcpt_read_temporal(None, None, None) == -1
    assert L.mcpt_temporal_info(None, None, None, None) == -1 and L.mcpt_last_temporal_ms(None, None, None) == -1
    assert mcpt_mod.NO_TEMPORAL == -10 and b"temporal" in L.mcpt_error_string(-10)
    assert [n for n, _ in mcpt_mod.TemporalRecord._fields_] == list(KEYS) + ["frames"]
    assert 1 <= mcpt_mod.TEMPORAL_MAX_HISTORY <= 65535 and mcpt_mod.TEMPORAL_PLANE_TOL > 0
    for meth in ("temporal_begin", "temporal_end", "temporal_accumulate", "denoise_temporal", "read_temporal",
                 "temporal_info", "render_frame_temporal", "last_temporal_ms"):
        assert callable(getattr(mcpt_mod.Renderer, meth))
    r = object.__new__(mcpt_mod.Renderer)           # no context: the checks below come before any call
    r._h = None
    cam = mcpt_mod.camera_canonical(8, 8)
    for spp, batches in ((4, 1), (1, 2), (4, 0)):
        with pytest.raises(mcpt_mod.MCPTError):
            r.render_frame_temporal(cam[0], cam[1], None, 1, spp, batches)
