// The adaptive checkpoint's file layer (csrc/mcpt_image.cpp: mcpt_adaptive_checkpoint_write /
// _read) under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU and without libmcpt:
// this program links mcpt_image.cpp alone (tests/test_adaptive_checkpoint_host.py builds and runs
// it).  It writes a small file, reads it back bit for bit, then reads every truncation of it: one
// cut per byte through the magic, the header and the tag, and one cut inside every later section
// (and one at each section's end).  The reader's arrays are allocated at exactly the sizes the
// header implies, so an over-read or over-write is a sanitizer report.  Exit 0 = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcpt.h"

// what mcpt_image.cpp takes from the rest of the library
int mcpt_err_bare(int status) { return status; }
namespace mcpt {
namespace host {
void transfo_translate(float, float, float, float*) {}
void transfo_scale(float, float, float, float*) {}
void transfo_rotate(int, float, float*) {}
void mat4_mul(const float*, const float*, float*) {}
}  // namespace host
}  // namespace mcpt

namespace {

int failures = 0;
void expect(bool ok, const char* what, long long at = -1) {
  if (ok) return;
  std::fprintf(stderr, "FAILED: %s (%lld)\n", what, at);
  ++failures;
}

std::vector<unsigned char> slurp(const std::string& path) {
  std::vector<unsigned char> out;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return out;
  unsigned char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

void spill(const std::string& path, const unsigned char* p, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(p, 1, n, f) != n) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    std::exit(3);
  }
  std::fclose(f);
}

struct Arrays {
  std::vector<int> active, passes;
  std::vector<float> accum, stats, emap;
  Arrays(size_t n_blocks, size_t n_px) : active(n_blocks), passes(n_blocks), accum(n_px * 3), stats(n_px * 4), emap(n_px * 2) {}
};

int read_all(const std::string& path, mcpt_adaptive_checkpoint_t* h, char* tag, Arrays& a, size_t n_px) {
  return mcpt_adaptive_checkpoint_read(path.c_str(), h, tag, a.active.data(), a.passes.data(), (long long)a.active.size(),
                                       a.accum.data(), a.stats.data(), a.emap.data(), (long long)n_px);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: adaptive_ckpt_sanitize DIR\n");
    return 2;
  }
  const std::string dir = argv[1], path = dir + "/a.ckpt", cut = dir + "/cut.ckpt";
  const int W = 11, rows = 9;   // 2 x 2 blocks, partial in both directions
  const size_t n_px = (size_t)W * rows, n_blocks = 4;
  mcpt_adaptive_checkpoint_t h;
  std::memset(&h, 0, sizeof(h));
  h.W = W; h.rows = rows; h.pass_count = 51; h.next_pass = 52; h.H = 37; h.rows_hash = 0x9e3779b97f4a7c15ull;
  h.p0 = 3; h.min_passes = 8; h.stats_passes = (1ll << 33) + 48; h.stats_batches = 5; h.emap_valid = 1;
  h.n_blocks = (int)n_blocks; h.blocks_x = 2;
  Arrays src(n_blocks, n_px);
  uint32_t seed = 12345u;
  auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed; };
  for (size_t b = 0; b < n_blocks; ++b) { src.active[b] = (int)(next() & 1u); src.passes[b] = (int)(next() % 97u); }
  for (float& v : src.accum) { const uint32_t u = next(); std::memcpy(&v, &u, 4); }   // any bits, NaNs included
  for (float& v : src.stats) { const uint32_t u = next(); std::memcpy(&v, &u, 4); }
  for (float& v : src.emap) { const uint32_t u = next(); std::memcpy(&v, &u, 4); }
  const char* tag = "scene=6 W=11 chunk=16 adaptive=0x1p-4";
  expect(mcpt_adaptive_checkpoint_write(path.c_str(), &h, tag, src.active.data(), src.passes.data(), src.accum.data(),
                                        src.stats.data(), src.emap.data()) == MCPT_OK, "write");

  // round trip
  {
    mcpt_adaptive_checkpoint_t g;
    std::vector<char> t(MCPT_CHECKPOINT_TAG_MAX);
    expect(mcpt_adaptive_checkpoint_read(path.c_str(), &g, t.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) ==
               MCPT_OK, "header-only read");
    expect(std::memcmp(&g, &h, sizeof(h)) == 0 && std::strcmp(t.data(), tag) == 0, "header fields");
    Arrays dst(n_blocks, n_px);
    expect(read_all(path, &g, t.data(), dst, n_px) == MCPT_OK, "full read");
    expect(std::memcmp(&g, &h, sizeof(h)) == 0 && std::strcmp(t.data(), tag) == 0, "header fields (full read)");
    expect(dst.active == src.active && dst.passes == src.passes, "block arrays");
    expect(std::memcmp(dst.accum.data(), src.accum.data(), n_px * 12) == 0, "accumulator bits");
    expect(std::memcmp(dst.stats.data(), src.stats.data(), n_px * 16) == 0, "statistics bits");
    expect(std::memcmp(dst.emap.data(), src.emap.data(), n_px * 8) == 0, "error map bits");
    // capacities one short, a partial set of arrays, NULL header and tag
    Arrays few(n_blocks - 1, n_px);
    expect(read_all(path, &g, t.data(), few, n_px) == MCPT_ERR_INVALID_ARG, "block capacity too small");
    expect(mcpt_adaptive_checkpoint_read(path.c_str(), &g, t.data(), dst.active.data(), dst.passes.data(), (long long)n_blocks,
                                         dst.accum.data(), dst.stats.data(), dst.emap.data(), (long long)n_px - 1) ==
               MCPT_ERR_INVALID_ARG, "pixel capacity too small");
    expect(mcpt_adaptive_checkpoint_read(path.c_str(), &g, t.data(), dst.active.data(), nullptr, (long long)n_blocks,
                                         dst.accum.data(), dst.stats.data(), dst.emap.data(), (long long)n_px) ==
               MCPT_ERR_INVALID_ARG, "partial set of arrays");
    expect(read_all(path, nullptr, nullptr, dst, n_px) == MCPT_OK, "read without header and tag");
  }

  // truncations
  const std::vector<unsigned char> data = slurp(path);
  const size_t tag_len = std::strlen(tag), fixed = 8 + 64;
  expect(data.size() == fixed + tag_len + n_blocks * 8 + n_px * 36, "file length", (long long)data.size());
  std::vector<size_t> cuts;
  for (size_t k = 0; k < fixed + tag_len; ++k) cuts.push_back(k);   // every byte of magic, header and tag
  size_t at = fixed + tag_len;
  for (size_t bytes : {n_blocks * 4, n_blocks * 4, n_px * 12, n_px * 16, n_px * 8}) {
    cuts.push_back(at);              // the section missing whole
    cuts.push_back(at + bytes / 2);  // cut inside it
    cuts.push_back(at + bytes - 1);  // its last byte missing
    at += bytes;
  }
  for (size_t k : cuts) {
    if (k >= data.size()) continue;
    spill(cut, data.data(), k);
    Arrays dst(n_blocks, n_px);
    mcpt_adaptive_checkpoint_t g;
    std::vector<char> t(MCPT_CHECKPOINT_TAG_MAX);
    expect(read_all(cut, &g, t.data(), dst, n_px) == MCPT_ERR_INVALID_ARG, "truncated file read in full", (long long)k);
    expect(mcpt_adaptive_checkpoint_read(cut.c_str(), &g, t.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) ==
               MCPT_ERR_INVALID_ARG, "truncated file, header only", (long long)k);
  }
  // a byte too many, a foreign magic, a plain checkpoint, a missing file
  {
    std::vector<unsigned char> more = data;
    more.push_back(0);
    spill(cut, more.data(), more.size());
    Arrays dst(n_blocks, n_px);
    expect(read_all(cut, nullptr, nullptr, dst, n_px) == MCPT_ERR_INVALID_ARG, "trailing byte");
    std::vector<unsigned char> foreign = data;
    foreign[6] = 'P'; foreign[7] = '2';
    spill(cut, foreign.data(), foreign.size());
    expect(read_all(cut, nullptr, nullptr, dst, n_px) == MCPT_ERR_INVALID_ARG, "MCPTCKP2 magic on an adaptive body");
    expect(mcpt_checkpoint_read(path.c_str(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
               MCPT_ERR_INVALID_ARG, "plain reader given an adaptive file");
    const std::string plain = dir + "/plain.ckpt";
    expect(mcpt_checkpoint_write(plain.c_str(), src.accum.data(), W, rows, 51, 52, tag) == MCPT_OK, "plain write");
    expect(read_all(plain, nullptr, nullptr, dst, n_px) == MCPT_ERR_INVALID_ARG, "adaptive reader given a plain file");
    expect(read_all(dir + "/missing.ckpt", nullptr, nullptr, dst, n_px) == MCPT_ERR_INVALID_ARG, "missing file");
  }
  // inconsistent headers are not written
  {
    mcpt_adaptive_checkpoint_t bad = h;
    bad.n_blocks = 5;
    expect(mcpt_adaptive_checkpoint_write(cut.c_str(), &bad, tag, src.active.data(), src.passes.data(), src.accum.data(),
                                          src.stats.data(), src.emap.data()) == MCPT_ERR_INVALID_ARG, "n_blocks of another grid");
    bad = h;
    bad.W = 0;
    expect(mcpt_adaptive_checkpoint_write(cut.c_str(), &bad, tag, src.active.data(), src.passes.data(), src.accum.data(),
                                          src.stats.data(), src.emap.data()) == MCPT_ERR_INVALID_ARG, "W = 0");
    // a header whose sizes lie about the body: the length check refuses it before any array is read
    std::vector<unsigned char> lie = data;
    const int32_t w2 = 19, nb2 = 6, bx2 = 3;
    std::memcpy(&lie[8], &w2, 4);
    std::memcpy(&lie[8 + 56], &nb2, 4);
    std::memcpy(&lie[8 + 60], &bx2, 4);
    spill(cut, lie.data(), lie.size());
    Arrays big(6, (size_t)19 * rows);
    expect(read_all(cut, nullptr, nullptr, big, (size_t)19 * rows) == MCPT_ERR_INVALID_ARG, "header larger than the body");
  }
  if (failures) return 1;
  std::printf("adaptive_ckpt_sanitize ok: %zu truncations\n", cuts.size());
  return 0;
}
