// mcpt.hpp — C++ host API over the libmcpt C ABI (include/mcpt.h), header-only.
//
// Mirrors the reference's host interface of the hot path so montecarlo.cpp-style code keeps
// its shape (names and argument meaning of bvh_gpu/scene.h, bvh_gpu/gpu_bvh_scene.h,
// easycppogl/gl_eigen.h):
//
//   GLVec4, GLMat4            Eigen column-major storage (gl_eigen.h:46-60)
//   Transfo::translate/scale/rotateX/rotateY/rotateZ   gl_eigen.cpp:29-105 (degrees)
//   Material (3 ctors + Material::light)               scene.h:30-49
//   PrimData, BB, Mesh/SP_Mesh                         scene.h:15-19, 64-73; mesh.h:85-96
//   ScenePrimitives: clear, nb, add_*, prim_data       scene.h:75-185
//   BVH_GPU_Scene(ScenePrimitives&): clear, add_sphere/add_cube/add_cylinder/add_cone/
//                  add_orientedQuad, add_mesh/place_mesh, finalize, depth(i), nb_prim,
//                  nb_emissives                                  gpu_bvh_scene.h:35-121
//   Renderer: the GL program + accumulation FBO of RTViewer (montecarlo.cpp:384-386, 408-477)
//
// Every matrix product goes through libmcpt (mcpt_mat4_mul) so transforms are bit-identical
// to the reference scenes the library builds.  Errors throw mcpt::Error (the reference has
// no error convention; the C ABI returns status codes).
#ifndef MCPT_HPP_
#define MCPT_HPP_

#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "mcpt.h"

namespace mcpt {

class Error : public std::runtime_error {
 public:
  Error(const std::string& what, int status)
      : std::runtime_error(what + " failed (" + std::to_string(status) + "): " + mcpt_error_string(status)),
        status_(status) {}
  int status() const { return status_; }

 private:
  int status_;
};

inline void check(int status, const char* what) {
  if (status != MCPT_OK) throw Error(what, status);
}

struct GLVec4 {
  float v[4];
  GLVec4(float r = 0, float g = 0, float b = 0, float a = 1) : v{r, g, b, a} {}
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};

// column-major 4x4 (Eigen default storage: m[col * 4 + row])
struct GLMat4 {
  float m[16];
  GLMat4() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = m[15] = 1.0f; }
  static GLMat4 Identity() { return GLMat4(); }
  float& operator()(int r, int c) { return m[c * 4 + r]; }
  float operator()(int r, int c) const { return m[c * 4 + r]; }
  const float* data() const { return m; }
  GLMat4 operator*(const GLMat4& b) const {
    GLMat4 r;
    check(mcpt_mat4_mul(m, b.m, r.m), "mcpt_mat4_mul");
    return r;
  }
  // mcpt_mat4_inverse (double arithmetic, rounded once); throws for a singular matrix
  GLMat4 inverse() const {
    GLMat4 r;
    check(mcpt_mat4_inverse(m, r.m), "mcpt_mat4_inverse");
    return r;
  }
};

namespace Transfo {
inline GLMat4 translate(float x, float y, float z) {
  GLMat4 r;
  check(mcpt_transfo_translate(x, y, z, r.m), "mcpt_transfo_translate");
  return r;
}
inline GLMat4 scale(float sx, float sy, float sz) {
  GLMat4 r;
  check(mcpt_transfo_scale(sx, sy, sz, r.m), "mcpt_transfo_scale");
  return r;
}
inline GLMat4 scale(float s) { return scale(s, s, s); }
inline GLMat4 rotateX(float deg) { GLMat4 r; check(mcpt_transfo_rotate(0, deg, r.m), "rotateX"); return r; }
inline GLMat4 rotateY(float deg) { GLMat4 r; check(mcpt_transfo_rotate(1, deg, r.m), "rotateY"); return r; }
inline GLMat4 rotateZ(float deg) { GLMat4 r; check(mcpt_transfo_rotate(2, deg, r.m), "rotateZ"); return r; }
}  // namespace Transfo

class Material {
 public:
  GLVec4 color_;
  float shininess_, roughness_, emissivity_;
  Material(const GLVec4& color, float shin, float rough, float emi)
      : color_(color), shininess_(shin), roughness_(rough), emissivity_(emi) {}
  Material(const GLVec4& color, float shin, float rough) : Material(color, shin, rough, 0.0f) {}
  explicit Material(const GLVec4& color) : Material(color, 0.0f, 0.0f, 0.0f) {}
  static Material light(const GLVec4& col, float emi) { return Material(col, 0.0f, 0.0f, emi); }
  // the 7 floats the C ABI takes: r, g, b, a(opacity), shininess, roughness, emissivity
  void pack(float out[7]) const {
    for (int k = 0; k < 4; ++k) out[k] = color_[k];
    out[4] = shininess_; out[5] = roughness_; out[6] = emissivity_;
  }
};

struct GLVec3 {
  float v[3];
  GLVec3(float x = 0, float y = 0, float z = 0) : v{x, y, z} {}
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};

// One primitive's record, member for member the reference's PrimData (scene.h:64-73): three
// column-major mat4 (transform, inverse, mesh-BB transform), type (.x type code, .y mesh line),
// colour RGBA (A = opacity), material (shininess, roughness, emissivity, area), padding.
// 16 RGBA32F texels: the tex_prim_ texel layout mcpt_upload_scene takes.
struct PrimData {
  GLMat4 transfo_;
  GLMat4 inv_transfo_;
  GLMat4 inv_mesh_bb_transfo_;
  GLVec4 type_;
  GLVec4 color_;
  GLVec4 mat_info;
  GLVec4 padding2_;
};
static_assert(sizeof(PrimData) == 64 * sizeof(float), "PrimData = 16 RGBA32F texels (scene.h:64-73)");

// BVH node box, the reference's BB (scene.h:15-19: GLVec3 min_, max_): the 2 RGB32F texels of
// tex_bb_ (gpu_bvh_scene.cpp:39-41) mcpt_upload_scene takes per node
struct BB {
  GLVec3 min_;
  GLVec3 max_;
};
static_assert(sizeof(BB) == 6 * sizeof(float), "BB = 2 RGB32F texels (scene.h:15-19)");

// The triangle-mesh data BVH_GPU_Scene::add_mesh reads from the reference's Mesh
// (easycppogl/mesh.h:85-96): positions, normals, triangle vertex indices, bounding box.
class Mesh {
 public:
  std::vector<GLVec3> vertices_;
  std::vector<GLVec3> normals_;
  std::vector<unsigned> tri_indices;
  bool has_bb_ = false;   // false: the vertices' bounding box
  BB bb_;
  int nb_vertices() const { return (int)vertices_.size(); }
  int nb_triangles() const { return (int)(tri_indices.size() / 3); }
};
using SP_Mesh = std::shared_ptr<Mesh>;

// ScenePrimitives (scene.h:75-185): the primitive list.  Owns the library's host scene; the
// records are built by libmcpt (add_prim's inverse and area, prim_bb, sortEmissiveFirst).
class ScenePrimitives {
 public:
  ScenePrimitives() { check(mcpt_scene_create(&s_), "mcpt_scene_create"); }
  ~ScenePrimitives() { mcpt_scene_destroy(s_); }
  ScenePrimitives(const ScenePrimitives&) = delete;
  ScenePrimitives& operator=(const ScenePrimitives&) = delete;

  void clear() { check(mcpt_scene_clear(s_), "mcpt_scene_clear"); }
  int nb() const { int n = 0; check(mcpt_scene_nb_prim(s_, &n), "mcpt_scene_nb_prim"); return n; }
  void add_sphere(const GLMat4& trf, const Material& mat) { add(&mcpt_scene_add_sphere, trf, mat, "add_sphere"); }
  void add_cube(const GLMat4& trf, const Material& mat) { add(&mcpt_scene_add_cube, trf, mat, "add_cube"); }
  void add_cylinder(const GLMat4& trf, const Material& mat) { add(&mcpt_scene_add_cylinder, trf, mat, "add_cylinder"); }
  void add_cone(const GLMat4& trf, const Material& mat) { add(&mcpt_scene_add_cone, trf, mat, "add_cone"); }
  void add_orientedQuad(const GLMat4& trf, const Material& mat) {
    add(&mcpt_scene_add_oriented_quad, trf, mat, "add_orientedQuad");
  }
  // ScenePrimitives::prim_data (scene.h:86-89): the records of a finalized scene, in order
  // (emissive first).  The pointer stays valid until the next prim_data() call.
  const PrimData* prim_data() const {
    const int n = nb(), d = depth_();
    prims_.assign((size_t)n, PrimData());
    std::vector<float> nodes(((size_t(2) << d) - 1) * 6);
    std::vector<int> leaves(size_t(1) << d);
    check(mcpt_scene_get_buffers(s_, reinterpret_cast<float*>(prims_.data()), nodes.data(), leaves.data()),
          "mcpt_scene_get_buffers");
    return prims_.data();
  }
  mcpt_scene* handle() const { return s_; }

 private:
  friend class BVH_GPU_Scene;
  typedef int (*AddFn)(mcpt_scene*, const float*, const float*);
  void add(AddFn fn, const GLMat4& trf, const Material& mat, const char* what) {
    float m7[7];
    mat.pack(m7);
    check(fn(s_, trf.m, m7), what);
  }
  int depth_() const { int d = 0; check(mcpt_scene_depth(s_, &d), "mcpt_scene_depth"); return d; }
  mcpt_scene* s_ = nullptr;
  mutable std::vector<PrimData> prims_;
};

// BVH_GPU_Scene (gpu_bvh_scene.h:35-121) over a caller-owned ScenePrimitives, as in RTViewer
// (montecarlo.cpp:92-93, 133: scene_ declared first, bvh_gpu_scene_(scene_)).  The default
// constructor owns its primitives (a convenience the reference does not have).  finalize()
// = sortEmissiveFirst + BVH_KDtree::init/compute (gpu_bvh_scene.cpp:121-129); the "textures"
// are the flat buffers Renderer::upload sends to the device.
class BVH_GPU_Scene {
 public:
  explicit BVH_GPU_Scene(ScenePrimitives& sc) : scene_(&sc) {}
  BVH_GPU_Scene() : own_(new ScenePrimitives()), scene_(own_.get()) {}
  BVH_GPU_Scene(const BVH_GPU_Scene&) = delete;
  BVH_GPU_Scene& operator=(const BVH_GPU_Scene&) = delete;

  // one of the 8 scenes of montecarlo.cpp:629-795 (keys Q..I = 1..8), finalized
  void build_reference(int scene_id, float light_intensity = 1.2f) {
    check(mcpt_scene_build_reference(s(), scene_id, light_intensity), "mcpt_scene_build_reference");
  }
  void clear() { scene_->clear(); }
  void add_sphere(const GLMat4& trf, const Material& mat) { scene_->add_sphere(trf, mat); }
  void add_cube(const GLMat4& trf, const Material& mat) { scene_->add_cube(trf, mat); }
  void add_cylinder(const GLMat4& trf, const Material& mat) { scene_->add_cylinder(trf, mat); }
  void add_cone(const GLMat4& trf, const Material& mat) { scene_->add_cone(trf, mat); }
  void add_orientedQuad(const GLMat4& trf, const Material& mat) { scene_->add_orientedQuad(trf, mat); }
  // add_mesh (gpu_bvh_scene.cpp:51-74): stores the mesh and builds its own BVH; returns its
  // index for place_mesh (gpu_bvh_scene.h:89-92), which adds an instance with a transform
  int add_mesh(const SP_Mesh& m) {
    // vertex normals are required (Mesh::compute_normals gives them; mesh_inter_geom_info reads them)
    if (!m || m->vertices_.empty() || m->normals_.size() != m->vertices_.size())
      throw Error("add_mesh (mesh needs vertices and one normal per vertex)", MCPT_ERR_INVALID_ARG);
    int id = -1;
    check(mcpt_scene_add_mesh(s(), m->vertices_[0].v, m->normals_[0].v, m->nb_vertices(),
                              m->tri_indices.data(), m->nb_triangles(),
                              m->has_bb_ ? m->bb_.min_.v : nullptr, &id),
          "mcpt_scene_add_mesh");
    return id;
  }
  void place_mesh(int i, const GLMat4& trf, const Material& mat) {
    float m7[7];
    mat.pack(m7);
    check(mcpt_scene_place_mesh(s(), i, trf.m, m7), "mcpt_scene_place_mesh");
  }
  // same-topology update of mesh i (no reference equivalent): m's vertices and normals replace the
  // mesh's and its BVH boxes are refitted; every vertex inside the bb the mesh was added with
  void update_mesh(int i, const SP_Mesh& m) {
    if (!m || m->vertices_.empty() || m->normals_.size() != m->vertices_.size())
      throw Error("update_mesh (mesh needs vertices and one normal per vertex)", MCPT_ERR_INVALID_ARG);
    check(mcpt_scene_update_mesh(s(), i, m->vertices_[0].v, m->normals_[0].v, m->nb_vertices()), "mcpt_scene_update_mesh");
  }
  // mesh i's tree rebuilt from its current vertices by stable median splits (mcpt_scene_rebuild_mesh);
  // tris (3 mesh-local vertex indices per triangle, the mesh's count) replaces its triangles first
  void rebuild_mesh(int i, const std::vector<unsigned>* tris = nullptr) {
    check(mcpt_scene_rebuild_mesh(s(), i, tris ? tris->data() : nullptr, tris ? (int)(tris->size() / 3) : 0),
          "mcpt_scene_rebuild_mesh");
  }
  // mesh i's first vertex in the flat vertex arrays (Renderer::update_mesh_vertices)
  int mesh_first_vertex(int i) const {
    int first = 0, n = 0;
    check(mcpt_scene_mesh_vertex_range(s(), i, &first, &n), "mcpt_scene_mesh_vertex_range");
    return first;
  }
  void finalize() { check(mcpt_scene_finalize(s()), "mcpt_scene_finalize"); }
  int depth(int /*bvh*/ = 0) const { return scene_->depth_(); }
  int nb_prim() const { return scene_->nb(); }
  int nb_emissives() const { int n = 0; check(mcpt_scene_nb_emissives(s(), &n), "mcpt_scene_nb_emissives"); return n; }
  int nb_meshes() const {
    int nm = 0, nn = 0, nl = 0, nt = 0, nv = 0;
    check(mcpt_scene_mesh_sizes(s(), &nm, &nn, &nl, &nt, &nv), "mcpt_scene_mesh_sizes");
    return nm;
  }

  // the reference's texture layouts (tex_prim / tex_bb / tex_ind), flattened
  void buffers(std::vector<float>& prims, std::vector<float>& nodes, std::vector<int>& leaves) const {
    const int n = nb_prim(), d = depth();
    prims.assign((size_t)n * 64, 0.0f);
    nodes.assign(((size_t(2) << d) - 1) * 6, 0.0f);
    leaves.assign(size_t(1) << d, 0);
    check(mcpt_scene_get_buffers(s(), prims.data(), nodes.data(), leaves.data()), "mcpt_scene_get_buffers");
  }
  // the root BVH_KDtree's data_BB() / data_ind() (bvh.h:36-44), typed
  void bvh(std::vector<BB>& bbs, std::vector<int>& ind) const {
    std::vector<float> p, n;
    buffers(p, n, ind);
    bbs.resize(n.size() / 6);
    for (size_t i = 0; i < bbs.size(); ++i) {
      bbs[i].min_ = GLVec3(n[i * 6], n[i * 6 + 1], n[i * 6 + 2]);
      bbs[i].max_ = GLVec3(n[i * 6 + 3], n[i * 6 + 4], n[i * 6 + 5]);
    }
  }
  ScenePrimitives& scene() const { return *scene_; }
  mcpt_scene* handle() const { return s(); }

 private:
  mcpt_scene* s() const { return scene_->s_; }
  std::unique_ptr<ScenePrimitives> own_;
  ScenePrimitives* scene_;
};

// canonical camera of RTViewer at aspect W/H: (P·V)^-1 and V^-1, column-major
struct Camera {
  GLMat4 invPV, invV;
  static Camera canonical(int W, int H) {
    Camera c;
    check(mcpt_camera_canonical(W, H, c.invPV.m, c.invV.m), "mcpt_camera_canonical");
    return c;
  }
  // the canonical camera with the world turned `deg` degrees about the scene's up axis (z): P·V
  // becomes P·V·R, so both inverses get R^-1 in front
  static Camera orbit(int W, int H, float deg) {
    const Camera c = canonical(W, H);
    const GLMat4 rinv = Transfo::rotateZ(-deg);
    Camera o;
    o.invPV = rinv * c.invPV;
    o.invV = rinv * c.invV;
    return o;
  }
  // the forward matrix P·V (what temporal_accumulate takes for the previous frame's camera)
  GLMat4 PV() const { return invPV.inverse(); }
};

// The loop behind Renderer::render_adaptive_until and mcpt_render's adaptive renders: every step is
// what mcpt_adaptive_until_next (mcpt.h) says follows `done` passes in `calls` render calls, issued as
// render(first, n), select() -> its record's n_active_blocks, or run(first, rounds) -> what the queued
// run did (null: never queued; render and select may be null where every step is a run); then
// after_step(done, calls) if given.  Ends at the cap, on a record with no active block or on a run
// that stopped short.  Unlike Python's driver it never selects on its own: when selects == 0 (fewer
// than two batches) the caller that needs a record owes the select.
struct AdaptiveRan { int rounds_run, selects_run; long long n_active; };   // n_active: the last record's, if any
struct AdaptiveUntil { int done, calls, selects; };
inline AdaptiveUntil adaptive_until(int first_pass, int batch, int max_passes, int check_every, int queued_rounds,
                                    const std::function<void(int, int)>& render, const std::function<long long()>& select,
                                    const std::function<AdaptiveRan(int, int)>& run = nullptr,
                                    const std::function<void(int, int)>& after_step = nullptr, int done = 0,
                                    int calls = 0) {
  AdaptiveUntil u{done, calls, 0};
  for (long long n_active = 1; n_active > 0;) {
    int rounds = 0, n = 0, sel = 0;
    check(mcpt_adaptive_until_next(u.done, u.calls, batch, max_passes, check_every, run ? queued_rounds : 0, &rounds, &n,
                                   &sel), "mcpt_adaptive_until_next");
    if (rounds == 0 && n == 0) break;
    AdaptiveRan got{1, sel, 0};   // (a single call is one round)
    if (rounds > 0) {
      got = run(first_pass + u.done, rounds);
    } else {
      render(first_pass + u.done, n);
      if (sel) got.n_active = select();
    }
    if (got.selects_run > 0) n_active = got.n_active;
    u = {u.done + (rounds > 0 ? got.rounds_run * batch : n), u.calls + got.rounds_run, u.selects + got.selects_run};
    if (after_step) after_step(u.done, u.calls);
    if (got.rounds_run < rounds) break;
  }
  return u;
}

// prg_ray + the RGB32F accumulation FBO (montecarlo.cpp:384-386, 408-477), one GPU
class Renderer {
 public:
  explicit Renderer(int device = 0) { check(mcpt_create(device, &c_), "mcpt_create"); }
  ~Renderer() { mcpt_destroy(c_); }
  Renderer(const Renderer&) = delete;
  Renderer& operator=(const Renderer&) = delete;

  // BVH_GPU_Scene::finalize's texture uploads (gpu_bvh_scene.cpp:121-187): primitives, root
  // BVH and, if the scene has mesh instances, the meshes and their BVHs
  void upload(const BVH_GPU_Scene& sc) {
    std::vector<float> p, n;
    std::vector<int> l;
    sc.buffers(p, n, l);
    check(mcpt_upload_scene(c_, p.data(), sc.nb_prim(), n.data(), l.data(), sc.depth(), sc.nb_emissives()),
          "mcpt_upload_scene");
    int nm = 0, nn = 0, nl = 0, nt = 0, nv = 0;
    check(mcpt_scene_mesh_sizes(sc.handle(), &nm, &nn, &nl, &nt, &nv), "mcpt_scene_mesh_sizes");
    if (nm > 0) {
      std::vector<int> info((size_t)nm * 4), leaves((size_t)nl), tris((size_t)nt * 3);
      std::vector<float> nodes((size_t)nn * 6), verts((size_t)nv * 3), norms((size_t)nv * 3);
      check(mcpt_scene_get_mesh_buffers(sc.handle(), info.data(), nodes.data(), leaves.data(), tris.data(),
                                        verts.data(), norms.data()),
            "mcpt_scene_get_mesh_buffers");
      check(mcpt_upload_meshes(c_, nm, info.data(), nn, nodes.data(), nl, leaves.data(), nt, tris.data(), nv,
                               verts.data(), norms.data()),
            "mcpt_upload_meshes");
      std::vector<int> counts((size_t)nm);   // (where each mesh's vertices lie: rebuild_mesh with new triangles)
      for (int m = 0, first = 0; m < nm; ++m)
        check(mcpt_scene_mesh_vertex_range(sc.handle(), m, &first, &counts[m]), "mcpt_scene_mesh_vertex_range");
      check(mcpt_set_mesh_vertex_counts(c_, nm, counts.data()), "mcpt_set_mesh_vertex_counts");
    }
  }
  // deforming meshes (mcpt.h): n x 3 positions and normals over the uploaded vertices from `first`
  // on (BVH_GPU_Scene::mesh_first_vertex), then the refit of mesh i's records (-1: every mesh's) on
  // the device; want_record waits once and fills the record
  void update_mesh_vertices(int first, const std::vector<GLVec3>& verts, const std::vector<GLVec3>& normals) {
    if (verts.empty() || normals.size() != verts.size())
      throw Error("update_mesh_vertices (one normal per vertex)", MCPT_ERR_INVALID_ARG);
    check(mcpt_update_mesh_vertices(c_, first, (int)verts.size(), verts[0].v, normals[0].v), "mcpt_update_mesh_vertices");
  }
  void update_mesh_vertices_device(int first, int n, const void* verts_dev, const void* normals_dev) {
    check(mcpt_update_mesh_vertices_device(c_, first, n, verts_dev, normals_dev), "mcpt_update_mesh_vertices_device");
  }
  mcpt_refit_t refit_mesh(int i = -1, bool want_record = true) {
    mcpt_refit_t rec{};
    check(mcpt_refit_mesh(c_, i, want_record ? &rec : nullptr), "mcpt_refit_mesh");
    return rec;
  }
  // mesh i's BVH (-1: every mesh's, without tris) rebuilt on the device: a new leaf order from the
  // current vertices, then the refit (mcpt_rebuild_mesh); tris as BVH_GPU_Scene::rebuild_mesh's
  mcpt_rebuild_t rebuild_mesh(int i = -1, const std::vector<int>* tris = nullptr, bool want_record = true) {
    mcpt_rebuild_t rec{};
    check(mcpt_rebuild_mesh(c_, i, tris ? tris->data() : nullptr, tris ? (int)(tris->size() / 3) : 0,
                            want_record ? &rec : nullptr), "mcpt_rebuild_mesh");
    return rec;
  }
  // the reference's own arrays, as BVH_GPU_Scene::finalize hands them to its textures:
  // ScenePrimitives::prim_data() (scene.h:86-89) and the root BVH_KDtree's data_BB() /
  // data_ind() / depth() (bvh.h:24-44) — no repacking on the host
  void upload(const PrimData* prims, int n_prims, const BB* bbs, const int* ind, int depth, int nb_emissives) {
    check(mcpt_upload_scene(c_, reinterpret_cast<const float*>(prims), n_prims, reinterpret_cast<const float*>(bbs),
                            ind, depth, nb_emissives),
          "mcpt_upload_scene");
  }
  void set_target(int W, int H, int band_rows = 8, int world = 1, int rank = 0) {
    check(mcpt_set_target(c_, W, H, band_rows, world, rank), "mcpt_set_target");
    W_ = W; H_ = H;
    check(mcpt_local_rows(c_, &rows_), "mcpt_local_rows");
  }
  // explicit shard: local row i renders global row rows[i]
  void set_target_rows(int W, int H, const std::vector<int>& rows) {
    check(mcpt_set_target_rows(c_, W, H, rows.data(), (int)rows.size()), "mcpt_set_target_rows");
    W_ = W; H_ = H; rows_ = (int)rows.size();
  }
  // this rank's rows of the balanced multi-GPU partition (mcpt_balanced_rows)
  static std::vector<int> balanced_rows(int H, int world, int rank, int band_rows = 8) {
    int n = 0;
    check(mcpt_balanced_rows(H, world, rank, band_rows, nullptr, &n), "mcpt_balanced_rows");
    std::vector<int> rows((size_t)n);
    check(mcpt_balanced_rows(H, world, rank, band_rows, rows.data(), &n), "mcpt_balanced_rows");
    return rows;
  }
  // global row ids of the local rows
  std::vector<int> local_row_ids() const {
    std::vector<int> rows((size_t)rows_);
    if (rows_) check(mcpt_local_row_ids(c_, rows.data()), "mcpt_local_row_ids");
    return rows;
  }
  // numero_pass = first_pass .. first_pass + n_passes - 1, accumulated (blend ONE/ONE)
  void render(const Camera& cam, int first_pass, int n_passes, float date, int bounces, float refract_ind,
              int variant = MCPT_MONTECARLO) {
    check(mcpt_render(c_, cam.invPV.m, cam.invV.m, first_pass, n_passes, date, bounces, refract_ind, variant),
          "mcpt_render");
  }
  void clear_accum() { check(mcpt_clear_accum(c_), "mcpt_clear_accum"); }
  // (local rows × W × 3 sums, pass count)
  int read_accum(std::vector<float>& rgb) const {
    rgb.assign((size_t)rows_ * W_ * 3, 0.0f);
    int n = 0;
    check(mcpt_read_accum(c_, rgb.data(), &n), "mcpt_read_accum");
    return n;
  }
  // the inverse of read_accum (resume): local rows × W × 3 sums holding `passes` passes
  void write_accum(const std::vector<float>& rgb, int passes) {
    if (rgb.size() != (size_t)rows_ * W_ * 3) throw Error("write_accum: wrong size", MCPT_ERR_INVALID_ARG);
    check(mcpt_write_accum(c_, rgb.data(), passes), "mcpt_write_accum");
  }
  // checkpoint / resume of a progressive render (mcpt_checkpoint_save / _load): the file holds
  // the sums, their pass count, the next call's first pass, a tag of the render parameters and
  // the target's identity (H, row ids)
  void save_checkpoint(const std::string& path, int next_pass, const std::string& tag) const {
    check(mcpt_checkpoint_save(c_, path.c_str(), next_pass, tag.c_str()), "mcpt_checkpoint_save");
  }
  // returns the next first pass; throws if the file belongs to another target / shard or its
  // tag differs from this render's
  int load_checkpoint(const std::string& path, const std::string& tag) {
    int next = 0;
    check(mcpt_checkpoint_load(c_, path.c_str(), tag.c_str(), &next), "mcpt_checkpoint_load");
    return next;
  }
  // fs_frag: the averaged image (single-shard target)
  std::vector<float> read_image() const {
    std::vector<float> acc;
    const int n = read_accum(acc);
    std::vector<float> img(acc.size());
    check(mcpt_average(acc.data(), (long long)acc.size(), n > 0 ? n : 1, img.data()), "mcpt_average");
    return img;
  }
  float last_render_ms() const { float ms = 0; check(mcpt_last_render_ms(c_, &ms), "mcpt_last_render_ms"); return ms; }
  // this (full-frame) renderer's accumulator <- the shards' rows (mcpt_gather_rows: peer copies
  // over xGMI inside one process; asynchronous, read_accum / read_image synchronize)
  void gather_rows(const std::vector<const Renderer*>& shards) {
    std::vector<mcpt_ctx*> h;
    for (const Renderer* r : shards) h.push_back(r->c_);
    check(mcpt_gather_rows(c_, h.data(), (int)h.size()), "mcpt_gather_rows");
  }
  // guide buffers (AOVs) of every local pixel's primary hit (mcpt_render_guides / mcpt_read_guides):
  // guide8 = local pixels x {N.xyz, key bits, P.xyz, dist}, albedo4 = local pixels x rgba
  void render_guides(const Camera& cam) {
    check(mcpt_render_guides(c_, cam.invPV.m, cam.invV.m), "mcpt_render_guides");
  }
  void read_guides(std::vector<float>& guide8, std::vector<float>& albedo4) const {
    guide8.assign((size_t)rows_ * W_ * 8, 0.0f);
    albedo4.assign((size_t)rows_ * W_ * 4, 0.0f);
    check(mcpt_read_guides(c_, guide8.data(), albedo4.data()), "mcpt_read_guides");
  }
  // the edge-avoiding a-trous filter over accum / pass_count (mcpt_denoise; full-frame targets,
  // after render_guides); the accumulator stays as it is.  Default sigmas: DESIGN.md §3.7
  static constexpr float kDenoiseSigmaColor = 4.0f, kDenoiseSigmaPlane = 1.0f;
  std::vector<float> denoise(int iterations = 5, float sigma_color = kDenoiseSigmaColor,
                             float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise(c_, iterations, sigma_color, sigma_plane), "mcpt_denoise");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  // (guides kernel ms, filter ms) of the last render_guides / denoise
  void last_denoise_ms(float& guides_ms, float& filter_ms) const {
    check(mcpt_last_denoise_ms(c_, &guides_ms, &filter_ms), "mcpt_last_denoise_ms");
  }
  // one iteration of the last denoise alone (-1: its averaging step), and which iterations staged
  // their taps in LDS (bit s)
  float denoise_iteration_ms(int iteration) const {
    float ms = 0; check(mcpt_denoise_iteration_ms(c_, iteration, &ms), "mcpt_denoise_iteration_ms"); return ms;
  }
  int last_denoise_path() const {
    int m = 0; check(mcpt_last_denoise_path(c_, &m), "mcpt_last_denoise_path"); return m;
  }
  // noise statistics, the convergence metric and the noise-guided filter (mcpt.h):
  // between stats_begin and stats_end every render call is one batch of the window
  static constexpr float kDenoiseKColor = 64.0f, kErrorMuFloor = 0.01f;
  // the variance filter's colour width in standard deviations of the carried variance
  static constexpr float kDenoiseKVariance = 16.0f;
  void stats_begin() { check(mcpt_stats_begin(c_), "mcpt_stats_begin"); }
  void stats_end() { check(mcpt_stats_end(c_), "mcpt_stats_end"); }
  void stats_add_batch(int n) { check(mcpt_stats_add_batch(c_, n), "mcpt_stats_add_batch"); }
  struct StatsInfo { bool on; long long passes; int batches; };
  StatsInfo stats_info() const {
    int on = 0, b = 0; long long n = 0;
    check(mcpt_stats_info(c_, &on, &n, &b), "mcpt_stats_info");
    return StatsInfo{on != 0, n, b};
  }
  mcpt_convergence_t convergence(float threshold, float mu_floor = kErrorMuFloor) {
    mcpt_convergence_t rec;
    check(mcpt_convergence(c_, threshold, mu_floor, &rec), "mcpt_convergence");
    return rec;
  }
  // local pixels x {se, r} of the last convergence()
  std::vector<float> read_error_map() const {
    std::vector<float> m((size_t)rows_ * W_ * 2);
    check(mcpt_read_error_map(c_, m.data()), "mcpt_read_error_map");
    return m;
  }
  std::vector<float> denoise_guided(int iterations = 5, float k_color = kDenoiseKColor,
                                    float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_guided(c_, iterations, k_color, sigma_plane), "mcpt_denoise_guided");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  // the variance-propagating filter (mcpt_denoise_variance): denoise_guided's preconditions; the
  // error map's variance is prefiltered 3x3, carried in the image's fourth word and filtered along
  std::vector<float> denoise_variance(int iterations = 5, float k_color = kDenoiseKVariance,
                                      float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_variance(c_, iterations, k_color, sigma_plane), "mcpt_denoise_variance");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  // local pixels x 1: the variance the last denoise_variance / denoise_resolved_variance carried
  std::vector<float> read_denoised_variance() const {
    std::vector<float> v((size_t)rows_ * W_);
    check(mcpt_read_denoised_variance(c_, v.data()), "mcpt_read_denoised_variance");
    return v;
  }
  void last_stats_ms(float& update_ms, float& error_ms) const {
    check(mcpt_last_stats_ms(c_, &update_ms, &error_ms), "mcpt_last_stats_ms");
  }
  // ---- temporal reprojection across camera moves (mcpt.h): the defaults are the
  // sweep's (tools/temporal_bench.py)
  static constexpr int kTemporalMaxHistory = 8;
  static constexpr float kTemporalPlaneTol = 0.01f;
  void temporal_begin() { check(mcpt_temporal_begin(c_), "mcpt_temporal_begin"); }
  void temporal_end() { check(mcpt_temporal_end(c_), "mcpt_temporal_end"); }
  // device ms of the last accumulate: its kernel and the guides' copy behind it (0: ping-pong)
  void last_temporal_ms(float& accumulate_ms, float& copy_ms) const {
    check(mcpt_last_temporal_ms(c_, &accumulate_ms, &copy_ms), "mcpt_last_temporal_ms");
  }
  // prevPV: the P·V of the camera the history was made with (null only while the history is empty)
  mcpt_temporal_t temporal_accumulate(const GLMat4* prevPV, int max_history = kTemporalMaxHistory,
                                      float plane_tol = kTemporalPlaneTol) {
    mcpt_temporal_t rec;
    check(mcpt_temporal_accumulate(c_, prevPV ? prevPV->m : nullptr, max_history, plane_tol, &rec),
          "mcpt_temporal_accumulate");
    return rec;
  }
  // the variance filter from the temporal image; read_denoised_variance() serves its variance
  std::vector<float> denoise_temporal(int iterations = 5, float k_color = kDenoiseKVariance,
                                      float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_temporal(c_, iterations, k_color, sigma_plane), "mcpt_denoise_temporal");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  // ---- temporal adaptive sampling (mcpt.h): render only the blocks the history
  // cannot carry.  kTemporalTarget: the sweep's default (tools/temporal_adaptive_bench.py)
  static constexpr float kTemporalTarget = 0.05f;
  // temporal_accumulate with every pixel's own sample count (the adaptive mode on; retired blocks allowed)
  mcpt_temporal_t temporal_accumulate_resolved(const GLMat4* prevPV, int max_history = kTemporalMaxHistory,
                                               float plane_tol = kTemporalPlaneTol) {
    mcpt_temporal_t rec;
    check(mcpt_temporal_accumulate_resolved(c_, prevPV ? prevPV->m : nullptr, max_history, plane_tol, &rec),
          "mcpt_temporal_accumulate_resolved");
    return rec;
  }
  // the select on the error of the blend temporal_accumulate_resolved would write now
  mcpt_adaptive_temporal_t adaptive_select_temporal(const GLMat4* prevPV, float threshold = kTemporalTarget,
                                                    int max_history = kTemporalMaxHistory,
                                                    float plane_tol = kTemporalPlaneTol,
                                                    float mu_floor = kErrorMuFloor) {
    mcpt_adaptive_temporal_t rec;
    check(mcpt_adaptive_select_temporal(c_, prevPV ? prevPV->m : nullptr, max_history, plane_tol, threshold, mu_floor,
                                        &rec),
          "mcpt_adaptive_select_temporal");
    return rec;
  }
  // adaptive_run whose selects are adaptive_select_temporal: one host wait for the whole run
  mcpt_adaptive_run_t adaptive_run_temporal(const Camera& cam, int first_pass, int n_passes, int rounds,
                                            int check_every, float threshold, const GLMat4* prevPV, float date,
                                            int bounces, float refract_ind,
                                            std::vector<mcpt_adaptive_temporal_t>& records,
                                            int variant = MCPT_MONTECARLO, int max_history = kTemporalMaxHistory,
                                            float plane_tol = kTemporalPlaneTol, float mu_floor = kErrorMuFloor) {
    mcpt_adaptive_run_t run;
    records.assign((size_t)(rounds > 0 ? rounds : 1), mcpt_adaptive_temporal_t{});
    check(mcpt_adaptive_run_temporal(c_, cam.invPV.m, cam.invV.m, first_pass, n_passes, rounds, check_every, threshold,
                                     mu_floor, prevPV ? prevPV->m : nullptr, max_history, plane_tol, date, bounces,
                                     refract_ind, variant, records.data(), (int)records.size(), &run),
          "mcpt_adaptive_run_temporal");
    records.resize((size_t)run.selects_run);
    return run;
  }
  // Render passes first_pass, first_pass + 1, ... in calls of `batch` passes until the mean relative
  // error is at most target_error or max_passes are rendered; the convergence is queried after every
  // check_every calls (and at the cap), the calls in between are queued without a wait.  Begins a
  // statistics window unless one is on.  Returns the last record; *rendered = this call's passes.
  mcpt_convergence_t render_until(const Camera& cam, float target_error, int batch = 32, int max_passes = 4096,
                                  int check_every = 4, int first_pass = 1, float date = 0.0f, int bounces = 3,
                                  float refract_ind = 1.0f, int variant = MCPT_MONTECARLO, int* rendered = nullptr,
                                  float mu_floor = kErrorMuFloor) {
    if (batch <= 0 || check_every <= 0 || max_passes <= 0 || !(target_error > 0.0f))
      throw std::runtime_error("render_until: batch, check_every, max_passes and target_error must be positive");
    if (!stats_info().on) stats_begin();
    mcpt_convergence_t rec;
    bool have = false;
    int done = 0;
    for (int calls = 1; done < max_passes; ++calls) {
      const int n = batch < max_passes - done ? batch : max_passes - done;
      render(cam, first_pass + done, n, date, bounces, refract_ind, variant);
      done += n;
      if ((calls % check_every == 0 || done >= max_passes) && stats_info().batches >= 2) {
        rec = convergence(target_error, mu_floor);
        have = true;
        if (rec.mean_r <= (double)target_error) break;
      }
    }
    if (!have) rec = convergence(target_error, mu_floor);   // (fewer than two batches: MCPT_ERR_NO_STATS)
    if (rendered) *rendered = done;
    return rec;
  }
  // adaptive sampling of 8x8 blocks (mcpt.h)
  void adaptive_begin(int min_passes = 0) { check(mcpt_adaptive_begin(c_, min_passes), "mcpt_adaptive_begin"); }
  void adaptive_end() { check(mcpt_adaptive_end(c_), "mcpt_adaptive_end"); }
  mcpt_adaptive_t adaptive_select(float threshold, float mu_floor = kErrorMuFloor) {
    mcpt_adaptive_t rec;
    check(mcpt_adaptive_select(c_, threshold, mu_floor, &rec), "mcpt_adaptive_select");
    return rec;
  }
  // the select on the denoised frame's error (mcpt_adaptive_select_filtered): the
  // map, denoise_resolved_variance(iterations, k_color, sigma_plane) on it, then the rule on the
  // filter's variance; read_denoised / read_denoised_variance return the filter's image.  Needs
  // render_guides.  raw_cap = 64: no guard on the raw error
  mcpt_adaptive_filtered_t adaptive_select_filtered(float threshold, float raw_cap = 64.0f,
                                                    float mu_floor = kErrorMuFloor, int iterations = 5,
                                                    float k_color = kDenoiseKVariance,
                                                    float sigma_plane = kDenoiseSigmaPlane) {
    mcpt_adaptive_filtered_t rec;
    check(mcpt_adaptive_select_filtered(c_, threshold, raw_cap, mu_floor, iterations, k_color, sigma_plane, &rec),
          "mcpt_adaptive_select_filtered");
    return rec;
  }
  // local pixels x 3: the last filter run's image
  std::vector<float> read_denoised() const {
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  struct AdaptiveInfo { bool on; long long n_active, n_blocks; };
  AdaptiveInfo adaptive_info() const {
    int on = 0; long long a = 0, b = 0;
    check(mcpt_adaptive_info(c_, &on, &a, &b), "mcpt_adaptive_info");
    return AdaptiveInfo{on != 0, a, b};
  }
  // the active block ids, ascending
  std::vector<int> read_active_blocks() const {
    std::vector<int> ids((size_t)adaptive_info().n_blocks + 1);
    int n = 0;
    check(mcpt_read_active_blocks(c_, ids.data(), (int)ids.size(), &n), "mcpt_read_active_blocks");
    ids.resize((size_t)n);
    return ids;
  }
  void render_adaptive(const Camera& cam, int first_pass, int n_passes, float date, int bounces, float refract_ind,
                       int variant = MCPT_MONTECARLO) {
    check(mcpt_render_adaptive(c_, cam.invPV.m, cam.invV.m, first_pass, n_passes, date, bounces, refract_ind, variant),
          "mcpt_render_adaptive");
  }
  // local pixels: every pixel's sample count / accum / (float)count
  std::vector<int> read_sample_counts() const {
    std::vector<int> n((size_t)rows_ * W_);
    check(mcpt_read_sample_counts(c_, n.data()), "mcpt_read_sample_counts");
    return n;
  }
  std::vector<float> read_resolved() const {
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_resolved(c_, img.data()), "mcpt_read_resolved");
    return img;
  }
  void last_adaptive_ms(float& select_ms, float& render_ms) const {
    check(mcpt_last_adaptive_ms(c_, &select_ms, &render_ms), "mcpt_last_adaptive_ms");
  }
  // Queued adaptive runs (mcpt_adaptive_run*): `rounds` rounds of {render_adaptive of
  // n_passes passes, on the schedule's rounds a select} on the device with one host wait, the bits of
  // that loop.  records: the selects' records in order (selects_run of them).
  mcpt_adaptive_run_t adaptive_run(const Camera& cam, int first_pass, int n_passes, int rounds, int check_every,
                                   float threshold, float date, int bounces, float refract_ind,
                                   std::vector<mcpt_adaptive_t>& records, int variant = MCPT_MONTECARLO,
                                   float mu_floor = kErrorMuFloor) {
    mcpt_adaptive_run_t run;
    records.assign((size_t)(rounds > 0 ? rounds : 1), mcpt_adaptive_t{});
    check(mcpt_adaptive_run(c_, cam.invPV.m, cam.invV.m, first_pass, n_passes, rounds, check_every, threshold, mu_floor,
                            date, bounces, refract_ind, variant, records.data(), (int)records.size(), &run),
          "mcpt_adaptive_run");
    records.resize((size_t)run.selects_run);
    return run;
  }
  mcpt_adaptive_run_t adaptive_run_filtered(const Camera& cam, int first_pass, int n_passes, int rounds,
                                            int check_every, float threshold, float raw_cap, int iterations, float date,
                                            int bounces, float refract_ind,
                                            std::vector<mcpt_adaptive_filtered_t>& records,
                                            int variant = MCPT_MONTECARLO, float mu_floor = kErrorMuFloor,
                                            float k_color = kDenoiseKVariance, float sigma_plane = kDenoiseSigmaPlane) {
    mcpt_adaptive_run_t run;
    records.assign((size_t)(rounds > 0 ? rounds : 1), mcpt_adaptive_filtered_t{});
    check(mcpt_adaptive_run_filtered(c_, cam.invPV.m, cam.invV.m, first_pass, n_passes, rounds, check_every, threshold,
                                     raw_cap, mu_floor, iterations, k_color, sigma_plane, date, bounces, refract_ind,
                                     variant, records.data(), (int)records.size(), &run),
          "mcpt_adaptive_run_filtered");
    records.resize((size_t)run.selects_run);
    return run;
  }
  // Begin a statistics window and the adaptive mode, render calls of `batch` passes for the active
  // blocks only, select after every check_every calls (from the second on, and at the cap) until no
  // block is active or max_passes are rendered.  The mode stays on (read_resolved, read_sample_counts).
  // queued_rounds K > 0: as queued runs of up to K rounds (adaptive_run), the same record and *rendered.
  mcpt_adaptive_t render_adaptive_until(const Camera& cam, float threshold, int batch = 32, int max_passes = 4096,
                                        int min_passes = 0, int check_every = 1, int first_pass = 1,
                                        float date = 0.0f, int bounces = 3, float refract_ind = 1.0f,
                                        int variant = MCPT_MONTECARLO, int* rendered = nullptr,
                                        float mu_floor = kErrorMuFloor, int queued_rounds = 0) {
    if (batch <= 0 || check_every <= 0 || max_passes <= 0 || !(threshold > 0.0f) || queued_rounds < 0)
      throw std::runtime_error("render_adaptive_until: batch, check_every, max_passes and threshold must be positive");
    stats_begin();
    adaptive_begin(min_passes);
    mcpt_adaptive_t rec;
    std::vector<mcpt_adaptive_t> recs;
    const AdaptiveUntil u = adaptive_until(
        first_pass, batch, max_passes, check_every, queued_rounds,
        [&](int first, int n) { render_adaptive(cam, first, n, date, bounces, refract_ind, variant); },
        [&] { return (rec = adaptive_select(threshold, mu_floor)).n_active_blocks; },
        [&](int first, int rounds) {
          const mcpt_adaptive_run_t got = adaptive_run(cam, first, batch, rounds, check_every, threshold, date, bounces,
                                                       refract_ind, recs, variant, mu_floor);
          return AdaptiveRan{got.rounds_run, got.selects_run, recs.empty() ? 0 : (rec = recs.back()).n_active_blocks};
        });
    if (u.selects == 0) rec = adaptive_select(threshold, mu_floor);   // (fewer than two batches: MCPT_ERR_NO_STATS)
    if (rendered) *rendered = u.done;
    return rec;
  }
  // frames with per-pixel sample counts (adaptive mode on, or after gather_rows_counted; mcpt.h,
  // DESIGN.md §3.9): denoise / denoise_guided over the resolved colour accum / (float)count
  std::vector<float> denoise_resolved(int iterations = 5, float sigma_color = kDenoiseSigmaColor,
                                      float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_resolved(c_, iterations, sigma_color, sigma_plane), "mcpt_denoise_resolved");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  std::vector<float> denoise_resolved_guided(int iterations = 5, float k_color = kDenoiseKColor,
                                             float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_resolved_guided(c_, iterations, k_color, sigma_plane), "mcpt_denoise_resolved_guided");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  std::vector<float> denoise_resolved_variance(int iterations = 5, float k_color = kDenoiseKVariance,
                                               float sigma_plane = kDenoiseSigmaPlane) {
    check(mcpt_denoise_resolved_variance(c_, iterations, k_color, sigma_plane), "mcpt_denoise_resolved_variance");
    std::vector<float> img((size_t)rows_ * W_ * 3);
    check(mcpt_read_denoised(c_, img.data()), "mcpt_read_denoised");
    return img;
  }
  // checkpoint / resume of an adaptive render (mcpt_adaptive_checkpoint_save / _load): the sums with
  // the statistics window, the error map and the blocks' state; the load turns statistics and the
  // adaptive mode on in the saved state and returns the next first pass
  void save_adaptive_checkpoint(const std::string& path, int next_pass, const std::string& tag) const {
    check(mcpt_adaptive_checkpoint_save(c_, path.c_str(), next_pass, tag.c_str()), "mcpt_adaptive_checkpoint_save");
  }
  int load_adaptive_checkpoint(const std::string& path, const std::string& tag) {
    int next = 0;
    check(mcpt_adaptive_checkpoint_load(c_, path.c_str(), tag.c_str(), &next), "mcpt_adaptive_checkpoint_load");
    return next;
  }
  // gather_rows for shards with per-pixel counts or different pass counts (mcpt_gather_rows_counted):
  // every frame row from exactly one shard; read_sample_counts / read_resolved / denoise_resolved
  // then serve this renderer
  void gather_rows_counted(const std::vector<const Renderer*>& shards) {
    std::vector<mcpt_ctx*> h;
    for (const Renderer* r : shards) h.push_back(r->c_);
    check(mcpt_gather_rows_counted(c_, h.data(), (int)h.size()), "mcpt_gather_rows_counted");
  }
  // the gathered error map (mcpt.h): after gather_rows / gather_rows_counted, the
  // shards' error maps (their last convergence() / adaptive_select()) into this full-frame renderer;
  // denoise_guided / denoise_resolved_guided, read_error_map and error_map_record then serve it
  void gather_error_map(const std::vector<const Renderer*>& shards) {
    std::vector<mcpt_ctx*> h;
    for (const Renderer* r : shards) h.push_back(r->c_);
    check(mcpt_gather_error_map(c_, h.data(), (int)h.size()), "mcpt_gather_error_map");
  }
  // its multi-process ends: local pixels x 8-byte {se, r} records into a device buffer / frame row y
  // from packed row src_row[y] (H ints, load_rows_counted's index)
  void pack_error_map_device(void* dst_dev, size_t bytes) {
    check(mcpt_pack_error_map_device(c_, dst_dev, bytes), "mcpt_pack_error_map_device");
  }
  void load_rows_error_map(const void* src_dev, long long src_rows, const std::vector<int>& src_row) {
    if ((int)src_row.size() != H_) throw std::runtime_error("load_rows_error_map: one source row per frame row");
    check(mcpt_load_rows_error_map(c_, src_dev, src_rows, src_row.data()), "mcpt_load_rows_error_map");
  }
  // convergence()'s record reduced from the stored r values of the map this renderer holds
  mcpt_convergence_t error_map_record(float threshold) {
    mcpt_convergence_t rec;
    check(mcpt_error_map_record(c_, threshold, &rec), "mcpt_error_map_record");
    return rec;
  }
  // 0 no error map, 1 the own window's, 2 the gathered map
  int error_map_source() const {
    int s = 0;
    check(mcpt_error_map_source(c_, &s), "mcpt_error_map_source");
    return s;
  }
  void set_traversal(int mode) { check(mcpt_set_traversal(c_, mode), "mcpt_set_traversal"); }
  // render lanes (consecutive launches overlapping each other's tails; same bits): on by default
  void set_render_lanes(bool on) { check(mcpt_set_render_lanes(c_, on ? 1 : 0), "mcpt_set_render_lanes"); }
  // stream schedule knobs (MCPT_TRAVERSAL_STREAM): path slots (0: default), refill threshold (-1: default)
  void set_stream_pool(int slots, int refill) { check(mcpt_set_stream_pool(c_, slots, refill), "mcpt_set_stream_pool"); }
  int width() const { return W_; }
  int height() const { return H_; }
  mcpt_ctx* handle() const { return c_; }

 private:
  mcpt_ctx* c_ = nullptr;
  int W_ = 0, H_ = 0, rows_ = 0;
};

inline void write_pfm(const std::string& path, const std::vector<float>& rgb, int W, int H) {
  check(mcpt_write_pfm(path.c_str(), rgb.data(), W, H), "mcpt_write_pfm");
}
inline void write_png(const std::string& path, const std::vector<float>& rgb, int W, int H) {
  check(mcpt_write_png(path.c_str(), rgb.data(), W, H), "mcpt_write_png");
}

}  // namespace mcpt

#endif  // MCPT_HPP_
