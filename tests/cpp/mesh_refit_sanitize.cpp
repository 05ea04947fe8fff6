// Stand-alone sanitizer program for the host refit (mcpt_scene_update_mesh, mcpt_scene_mesh_vertex_range):
// links mcpt_scene.cpp alone, built with -fsanitize=address,undefined and run on the CPU
// (tests/test_mesh_refit_sanitize.py).  Meshes of 1, 2, 3, 5 and 600 triangles: an update with the
// mesh's own vertices keeps every buffer, a deformation keeps every box around its triangles, and
// the refusals change nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mcpt.h"

int mcpt_err_bare(int status) { return status; }

struct Buffers {
  std::vector<int> info, leaves, tris;
  std::vector<float> nodes, verts, normals;
  bool operator==(const Buffers& o) const {
    auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
      return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
    };
    return info == o.info && leaves == o.leaves && tris == o.tris && same(nodes, o.nodes) && same(verts, o.verts) &&
           same(normals, o.normals);
  }
};

static Buffers fetch(mcpt_scene* s) {
  int nm = 0, nn = 0, nl = 0, nt = 0, nv = 0;
  mcpt_scene_mesh_sizes(s, &nm, &nn, &nl, &nt, &nv);
  Buffers b;
  b.info.resize((size_t)nm * 4); b.nodes.resize((size_t)nn * 6); b.leaves.resize(nl); b.tris.resize((size_t)nt * 3);
  b.verts.resize((size_t)nv * 3); b.normals.resize((size_t)nv * 3);
  mcpt_scene_get_mesh_buffers(s, b.info.data(), b.nodes.data(), b.leaves.data(), b.tris.data(), b.verts.data(),
                              b.normals.data());
  return b;
}

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void one(int n_tris) {
  const int nv = n_tris + 2;
  std::vector<float> v((size_t)nv * 3), n((size_t)nv * 3, 0.5f);
  for (int i = 0; i < nv * 3; ++i) v[i] = std::sin(0.7f * (float)i + (float)n_tris);
  std::vector<unsigned> t((size_t)n_tris * 3);
  for (int i = 0; i < n_tris; ++i) { t[3 * i] = i; t[3 * i + 1] = i + 1; t[3 * i + 2] = i + 2; }
  const float bb[6] = {-2, -2, -2, 2, 2, 2};
  mcpt_scene* s = nullptr;
  EXPECT(mcpt_scene_create(&s) == MCPT_OK);
  int id = -1;
  EXPECT(mcpt_scene_add_mesh(s, v.data(), n.data(), nv, t.data(), n_tris, bb, &id) == MCPT_OK && id == 0);
  const Buffers before = fetch(s);
  EXPECT(mcpt_scene_update_mesh(s, 0, v.data(), n.data(), nv) == MCPT_OK);
  EXPECT(fetch(s) == before);
  int first = -1, count = -1;
  EXPECT(mcpt_scene_mesh_vertex_range(s, 0, &first, &count) == MCPT_OK && first == 0 && count == nv);
  EXPECT(mcpt_scene_mesh_vertex_range(s, 1, &first, &count) == MCPT_ERR_INVALID_ARG);
  // refusals: a vertex outside the box, a NaN, a wrong count, a wrong id, a null array
  std::vector<float> bad = v;
  bad[4] = 2.5f;
  EXPECT(mcpt_scene_update_mesh(s, 0, bad.data(), n.data(), nv) == MCPT_ERR_BAD_SCENE);
  bad[4] = NAN;
  EXPECT(mcpt_scene_update_mesh(s, 0, bad.data(), n.data(), nv) == MCPT_ERR_BAD_SCENE);
  EXPECT(mcpt_scene_update_mesh(s, 0, v.data(), n.data(), nv - 1) == MCPT_ERR_INVALID_ARG);
  EXPECT(mcpt_scene_update_mesh(s, 1, v.data(), n.data(), nv) == MCPT_ERR_INVALID_ARG);
  EXPECT(mcpt_scene_update_mesh(s, 0, nullptr, n.data(), nv) == MCPT_ERR_INVALID_ARG);
  EXPECT(fetch(s) == before);
  // a deformation: every leaf's box holds its triangle, every parent its children
  std::vector<float> v2 = v;
  for (int i = 0; i < nv * 3; ++i) v2[i] = 0.9f * v[i] + 0.3f * std::cos(1.3f * (float)i);
  EXPECT(mcpt_scene_update_mesh(s, 0, v2.data(), n.data(), nv) == MCPT_OK);
  const Buffers b = fetch(s);
  const int d = b.info[2], nl = 1 << d;
  EXPECT(b.leaves == before.leaves && b.tris == before.tris);
  for (int k = 0; k < nl && d > 0; ++k) {
    const int tri = b.leaves[k];
    if (tri < 0) continue;
    const float* box = &b.nodes[(size_t)(nl - 1 + k) * 6];
    for (int c = 0; c < 3; ++c)
      for (int q = 0; q < 3; ++q) {
        const float x = v2[(size_t)t[3 * tri + c] * 3 + q];
        EXPECT(box[q] < x && x < box[3 + q]);
      }
  }
  for (int i = 0; i + 1 < nl; ++i)
    for (int child = 2 * i + 1; child <= 2 * i + 2; ++child)
      for (int q = 0; q < 3; ++q) {
        EXPECT(b.nodes[(size_t)i * 6 + q] <= b.nodes[(size_t)child * 6 + q]);
        EXPECT(b.nodes[(size_t)i * 6 + 3 + q] >= b.nodes[(size_t)child * 6 + 3 + q]);
      }
  mcpt_scene_destroy(s);
  std::printf("mesh of %d triangles: %s\n", n_tris, fails ? "FAILED" : "ok");
}

int main() {
  for (int n : {1, 2, 3, 5, 600}) one(n);
  return fails ? 1 : 0;
}
