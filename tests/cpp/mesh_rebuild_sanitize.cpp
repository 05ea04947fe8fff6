// Stand-alone sanitizer program for the host rebuild (mcpt_scene_rebuild_mesh): links mcpt_scene.cpp
// alone, built with -fsanitize=address,undefined and run on the CPU (tests/test_rebuild_plan_host.py).
// Meshes of 1, 2, 3, 4, 5, 7, 37 (copies of one triangle), 257, 600 and 1000 triangles: the rebuild
// keeps the sizes and every triangle in exactly one leaf, is idempotent, takes new rows, and its
// refusals change nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mcpt.h"

int mcpt_err_bare(int status) { return status; }

struct Buffers {
  std::vector<int> info, leaves, tris;
  std::vector<float> nodes, verts;
  bool operator==(const Buffers& o) const {
    auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
      return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
    };
    return info == o.info && leaves == o.leaves && tris == o.tris && same(nodes, o.nodes) && same(verts, o.verts);
  }
};

static Buffers fetch(mcpt_scene* s) {
  int nm = 0, nn = 0, nl = 0, nt = 0, nv = 0;
  mcpt_scene_mesh_sizes(s, &nm, &nn, &nl, &nt, &nv);
  Buffers b;
  b.info.resize((size_t)nm * 4); b.nodes.resize((size_t)nn * 6); b.leaves.resize(nl); b.tris.resize((size_t)nt * 3);
  b.verts.resize((size_t)nv * 3);
  mcpt_scene_get_mesh_buffers(s, b.info.data(), b.nodes.data(), b.leaves.data(), b.tris.data(), b.verts.data(), nullptr);
  return b;
}

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void one(int n_tris, bool copies) {
  const int nv = copies ? 3 : n_tris + 2;
  std::vector<float> v((size_t)nv * 3), n((size_t)nv * 3, 0.5f);
  for (int i = 0; i < nv * 3; ++i) v[i] = std::sin(0.7f * (float)i + (float)n_tris);
  std::vector<unsigned> t((size_t)n_tris * 3);
  for (int i = 0; i < n_tris; ++i)
    for (int k = 0; k < 3; ++k) t[3 * i + k] = copies ? k : i + k;
  const float bb[6] = {-2, -2, -2, 2, 2, 2};
  mcpt_scene* s = nullptr;
  EXPECT(mcpt_scene_create(&s) == MCPT_OK);
  int id = -1;
  EXPECT(mcpt_scene_add_mesh(s, v.data(), n.data(), nv, t.data(), n_tris, bb, &id) == MCPT_OK && id == 0);
  const Buffers added = fetch(s);
  EXPECT(mcpt_scene_rebuild_mesh(s, 0, nullptr, 0) == MCPT_OK);
  const Buffers b = fetch(s);
  EXPECT(b.info == added.info && b.tris == added.tris && b.leaves.size() == added.leaves.size());
  std::vector<int> seen(n_tris, 0);
  for (int tri : b.leaves)
    if (tri >= 0) { EXPECT(tri < n_tris); if (tri < n_tris) ++seen[tri]; }
  if (n_tris > 1) EXPECT(std::count(seen.begin(), seen.end(), 1) == n_tris);
  if (copies) {   // all keys equal: the order stays
    int next = 0;
    for (int tri : b.leaves)
      if (tri >= 0) EXPECT(tri == next++);
  }
  EXPECT(mcpt_scene_rebuild_mesh(s, 0, nullptr, 0) == MCPT_OK);
  EXPECT(fetch(s) == b);
  // refusals: a wrong id, a wrong count, an index outside the vertices
  std::vector<unsigned> bad = t;
  bad[bad.size() - 1] = (unsigned)nv;
  EXPECT(mcpt_scene_rebuild_mesh(s, 1, nullptr, 0) == MCPT_ERR_INVALID_ARG);
  EXPECT(mcpt_scene_rebuild_mesh(s, -1, nullptr, 0) == MCPT_ERR_INVALID_ARG);
  EXPECT(mcpt_scene_rebuild_mesh(s, 0, t.data(), n_tris + 1) == MCPT_ERR_INVALID_ARG);
  EXPECT(mcpt_scene_rebuild_mesh(s, 0, bad.data(), n_tris) == MCPT_ERR_INVALID_ARG);
  EXPECT(fetch(s) == b);
  // new rows: the triangles reversed
  std::vector<unsigned> t2((size_t)n_tris * 3);
  for (int i = 0; i < n_tris; ++i)
    for (int k = 0; k < 3; ++k) t2[3 * i + k] = t[3 * (size_t)(n_tris - 1 - i) + k];
  EXPECT(mcpt_scene_rebuild_mesh(s, 0, t2.data(), n_tris) == MCPT_OK);
  const Buffers c = fetch(s);
  EXPECT(c.info == b.info);
  for (size_t i = 0; i < t2.size(); ++i) EXPECT(c.tris[i] == (int)t2[i]);
  mcpt_scene_destroy(s);
  std::printf("mesh of %d triangles: %s\n", n_tris, fails ? "FAILED" : "ok");
}

int main() {
  for (int n : {1, 2, 3, 4, 5, 7, 257, 600, 1000}) one(n, false);
  one(37, true);
  return fails ? 1 : 0;
}
