"""C++ host side: include/mcpt.hpp (the reference-shaped C++ API) compiled against libmcpt,
the headless entry point, and the output step's image writers (PFM, PNG)."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "montecarlo-pathtracing_amd", "mcpt")


@pytest.fixture(scope="module")
def host_test_bin(tmp_path_factory, mcpt_mod):
    out = str(tmp_path_factory.mktemp("cpp") / "host_api_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "host_api_test.cpp"), "-o", out, "-L", LIBDIR, "-lmcpt",
                    f"-Wl,-rpath,{LIBDIR}"], check=True)
    return out


def test_cpp_scene_api_matches_reference_build(host_test_bin):
    r = subprocess.run([host_test_bin], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": ok") >= 6, r.stdout


def test_transfo_matches_scene_producer(mcpt_mod):
    T = mcpt_mod.Transfo
    m = T.mul(T.translate(200, 0, 100), T.rotateY(-110), T.scale(20, 20, 1))
    sc = mcpt_mod.Scene.reference(6)
    prims, _, _ = sc.buffers()
    light = prims[0]                       # emissive first (sortEmissiveFirst)
    assert light[58] > 0
    assert np.array_equal(m.view(np.uint32), light[:16].view(np.uint32))


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        assert scale < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)


def read_png_rgb8(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ = data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + body), typ
        chunks.setdefault(typ, b"")
        chunks[typ] += body
        pos += 12 + n
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, ctype) == (8, 2)
    raw = zlib.decompress(chunks[b"IDAT"])          # checks adler32
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_image_writers(mcpt_mod, tmp_path):
    rng = np.random.default_rng(3)
    H, W = 37, 300                                   # 300*3+1 = 901 B rows; > 65535 B in total
    img = rng.uniform(-0.5, 1.5, (H, W, 3)).astype(np.float32)
    img[0, 0] = [np.nan, np.inf, -np.inf]
    acc = img * np.float32(7)
    avg = mcpt_mod.average(acc, 7)
    assert np.array_equal(avg.view(np.uint32), (acc / np.float32(7)).view(np.uint32))
    mcpt_mod.write_pfm(str(tmp_path / "a.pfm"), img)
    back = read_pfm(str(tmp_path / "a.pfm"))
    assert np.array_equal(back.view(np.uint32), img.view(np.uint32))
    mcpt_mod.write_png(str(tmp_path / "a.png"), img)
    px = read_png_rgb8(str(tmp_path / "a.png"))
    want = np.where(np.nan_to_num(img, nan=0.0) > 0, np.round(np.clip(np.nan_to_num(img, nan=0.0, posinf=1.0), 0, 1)
                                                              * 255.0), 0).astype(np.uint8)[::-1]
    assert np.array_equal(px, want)


def test_headless_app_fails_loudly_without_gpu(mcpt_mod):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    if not os.path.exists(app):
        pytest.skip("mcpt_render not built")
    r = subprocess.run([app, "--scene", "6", "--width", "32", "--height", "24", "--spp", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "mcpt_create" in r.stderr


@pytest.mark.gpu
def test_cpp_host_renders_on_gpu(host_test_bin):
    r = subprocess.run([host_test_bin, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu image sum" in r.stdout
    assert "gpu reference-layout upload bit-equal: ok" in r.stdout, r.stdout


@pytest.mark.gpu
def test_cpp_render_adaptive_until_queued_equals_single(host_test_bin):
    """Renderer::render_adaptive_until (C++) with queued_rounds 3 and 0: the same resolved bits, sample
    counts, record and passes (host_api_test.cpp, mode gpu_until), under a time limit of its own."""
    r = subprocess.run([host_test_bin, "gpu_until"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    until = [ln for ln in r.stdout.splitlines() if ln.startswith("gpu adaptive until queued == single")]
    assert len(until) == 1 and until[0].endswith(": ok"), r.stdout


@pytest.mark.gpu
def test_headless_app_matches_oracle(oracle_mod, tmp_path):
    """mcpt_render --pfm output == fs_frag(oracle accumulation), bit for bit."""
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    W, H, S, B = 48, 40, 5, 8
    pfm = str(tmp_path / "s6.pfm")
    r = subprocess.run([app, "--scene", "6", "--width", str(W), "--height", str(H), "--spp", str(S), "--chunk", "2",
                        "--bounces", str(B), "--pfm", pfm, "--out", str(tmp_path / "s6.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = read_pfm(pfm)
    prims, nodes, leaves, d, _ = oracle_mod.scene(6)
    ipv, iv = oracle_mod.camera(W, H)
    acc = np.zeros((H, W, 3), np.float32)
    for first, n in ((1, 2), (3, 2), (5, 1)):     # the app's launches (--chunk 2), same accumulator
        oracle_mod.render(prims, nodes, leaves, d, ipv, iv, W, H, first, n, 0.0, B, 1.0, 0, accum=acc)
    assert np.array_equal(img.view(np.uint32), (acc / np.float32(S)).view(np.uint32))


@pytest.mark.gpu
def test_headless_app_stream_schedule_multi_device(oracle_mod, tmp_path):
    """mcpt_render --traversal stream on scene 8 with two shard contexts (each runs its own slot
    pools and streams; the shards' host threads share cuda:0): bit-equal to the oracle."""
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    W, H, S, B = 40, 32, 5, 12
    pfm = str(tmp_path / "s8.pfm")
    r = subprocess.run([app, "--scene", "8", "--width", str(W), "--height", str(H), "--spp", str(S), "--chunk", "2",
                        "--bounces", str(B), "--traversal", "stream", "--devices", "0,0", "--pfm", pfm],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = read_pfm(pfm)
    prims, nodes, leaves, d, _ = oracle_mod.scene(8)
    ipv, iv = oracle_mod.camera(W, H)
    acc = np.zeros((H, W, 3), np.float32)
    for first, n in ((1, 2), (3, 2), (5, 1)):
        oracle_mod.render(prims, nodes, leaves, d, ipv, iv, W, H, first, n, 0.0, B, 1.0, 0, accum=acc)
    assert np.array_equal(img.view(np.uint32), (acc / np.float32(S)).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "0,0,0", "0,0,0,0,0,0,0,0"])
def test_headless_app_multi_device_bit_equal(oracle_mod, tmp_path, devices):
    """mcpt_render --devices: one host thread per shard context (here all on cuda:0), balanced
    row shards, rows gathered device to device into a full frame (mcpt_gather_rows) — the
    output is bit-equal to the one-GPU render and to the oracle."""
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    W, H, S, B = 40, 53, 5, 8
    base = ["--scene", "6", "--width", str(W), "--height", str(H), "--spp", str(S), "--chunk", "2",
            "--bounces", str(B)]
    one, many = str(tmp_path / "one.pfm"), str(tmp_path / "many.pfm")
    r1 = subprocess.run([app] + base + ["--pfm", one], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0, r1.stderr
    rn = subprocess.run([app] + base + ["--pfm", many, "--devices", devices], capture_output=True, text=True,
                        timeout=120)
    assert rn.returncode == 0, rn.stderr
    rec = json.loads(rn.stdout.strip().splitlines()[-1])
    assert len(rec["shard_kernel_ms"]) == len(devices.split(",")) and rec["gather_ms"] >= 0
    a, b = read_pfm(one), read_pfm(many)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    prims, nodes, leaves, d, _ = oracle_mod.scene(6)
    ipv, iv = oracle_mod.camera(W, H)
    acc = np.zeros((H, W, 3), np.float32)
    for first, n in ((1, 2), (3, 2), (5, 1)):
        oracle_mod.render(prims, nodes, leaves, d, ipv, iv, W, H, first, n, 0.0, B, 1.0, 0, accum=acc)
    assert np.array_equal(b.view(np.uint32), (acc / np.float32(S)).view(np.uint32))
