// Mesh preparation: the caller's meshes -> the arrays the raster kernels read.  Host only, standard
// C++17, no HIP: rbsensor_capi.hip calls prepare_mesh() once per handle and uploads the vectors;
// tests/cpp/mesh_prep_check.cpp runs the same function on a CPU (tests/test_mesh_prep_cpu.py).
//
// The order of the floating-point operations is part of the contract: every output is held, bit for
// bit, to recorded values (tests/golden/mesh_prep.json).  Compile with -ffp-contract=off.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace rbs {

constexpr int kMeshMaxBodies = 16;          // == kMaxBodies of the kernels (asserted in rbs_handle.h)
constexpr int kMeshOk = 0;
constexpr int kMeshInvalidArgument = -1;    // == RBS_ERR_INVALID_ARGUMENT (asserted in rbs_handle.h)

struct MeshInput {                  // as in rbs_config
    int n_bodies;
    const double* vertices;         // concatenated xyz per body
    const int32_t* vertex_counts;   // [n_bodies]
    const int32_t* triangles;       // concatenated vertex-index triples, local to each body
    const int32_t* triangle_counts; // [n_bodies]
};

struct PreparedMesh {
    int tri_begin[kMeshMaxBodies + 1];   // triangle range per body (multiples of 64)
    int tri_end[kMeshMaxBodies];         // end of the body's REAL triangles (the rest of its last cluster is NaN padding)
    int vtx_begin[kMeshMaxBodies + 1];   // vertex range per body
    int body_cull[kMeshMaxBodies];       // 0: keep every triangle; +1/-1: closed, consistently wound, that winding is outward
    double sphere[kMeshMaxBodies][4];    // model-space bounding sphere: centre xyz, radius
    size_t n_alloc;                      // triangles in the soup, padding included (>= 64)
    int max_clusters;                    // the largest cluster count of any body
    std::vector<double> soup;            // [9][n_alloc] SoA: vertex k, coordinate c of triangle t at (3 k + c) * n_alloc + t
    std::vector<float> cluster_sphere;   // [clusters][4] centre xyz, radius
    std::vector<float> cluster_cone;     // [clusters][4] axis xyz, min cos (-2: never culled)
    std::vector<float> tri_plane;        // [n_alloc][4] unit normal, offset (NaN: never pre-culled)
    std::vector<double> cluster_vtx;     // [clusters][3][64] unique vertices of each cluster
    std::vector<int> cluster_nv;         // [clusters] how many (0: the cluster is set up per triangle)
    std::vector<unsigned> tri_local;     // [n_alloc] a triangle's three positions in its cluster's list, 8 bits each
    std::vector<float> vtx;              // [sum of vertex counts][4] float32 vertices
};

namespace mesh_detail {

static inline std::string fmt(const char* f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

static inline int fail(std::string* err, const std::string& msg)
{
    if (err) *err = msg;
    return kMeshInvalidArgument;
}

// n3 = (p1 - p0) x (p2 - p0); returns its length
static inline double tri_normal(const double* p0, const double* p1, const double* p2, double n3[3])
{
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    n3[0] = e1[1] * e2[2] - e1[2] * e2[1]; n3[1] = e1[2] * e2[0] - e1[0] * e2[2]; n3[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return std::sqrt(n3[0] * n3[0] + n3[1] * n3[1] + n3[2] * n3[2]);
}

// the three vertices of soup triangle t
static inline void soup_triangle(const PreparedMesh& m, size_t t, double p[3][3])
{
    for (int k = 0; k < 3; ++k)
        for (int c3 = 0; c3 < 3; ++c3) p[k][c3] = m.soup[(size_t)(3 * k + c3) * m.n_alloc + t];
}

// Back-face culling is exact only for a closed, consistently oriented surface: after
// welding vertices by position and dropping degenerate triangles every directed edge
// must occur exactly once, and its reverse exactly once.  The sign of the signed volume
// tells which winding is outward.  Returns +1 / -1, or 0: not such a surface.
static inline int closed_surface_sign(const double* V, int nv, const int32_t* T, int nt, const double ctr[3])
{
    std::map<std::array<double, 3>, int> weld;
    std::vector<int> wid(nv);
    for (int i = 0; i < nv; ++i) {
        const std::array<double, 3> key = {V[3 * i] + 0.0, V[3 * i + 1] + 0.0, V[3 * i + 2] + 0.0};  // -0 -> +0
        wid[i] = weld.emplace(key, (int)weld.size()).first->second;
    }
    std::map<std::pair<int, int>, int> edges;
    double vol6 = 0.0, avol6 = 0.0;
    bool ok = true;
    // connected components (shells) over the welded vertices: every shell must be wound the
    // same way -- an inside-out shell beside an outward one would pass the edge test and
    // still show the camera its "back" faces first
    std::vector<int> comp(weld.size());
    for (size_t i = 0; i < comp.size(); ++i) comp[i] = (int)i;
    auto find = [&](int x) { while (comp[x] != x) { comp[x] = comp[comp[x]]; x = comp[x]; } return x; };
    std::vector<double> tri_vol(nt, 0.0);
    for (int t = 0; t < nt && ok; ++t) {
        const int a = wid[T[3 * t]], bb = wid[T[3 * t + 1]], c3 = wid[T[3 * t + 2]];
        if (a == bb || bb == c3 || a == c3) continue;
        for (const auto& e : {std::make_pair(a, bb), std::make_pair(bb, c3), std::make_pair(c3, a)})
            if (++edges[e] > 1) ok = false;
        const double* p0 = V + 3 * T[3 * t]; const double* p1 = V + 3 * T[3 * t + 1]; const double* p2 = V + 3 * T[3 * t + 2];
        const double d = (p0[0] - ctr[0]) * ((p1[1] - ctr[1]) * (p2[2] - ctr[2]) - (p1[2] - ctr[2]) * (p2[1] - ctr[1])) -
                         (p0[1] - ctr[1]) * ((p1[0] - ctr[0]) * (p2[2] - ctr[2]) - (p1[2] - ctr[2]) * (p2[0] - ctr[0])) +
                         (p0[2] - ctr[2]) * ((p1[0] - ctr[0]) * (p2[1] - ctr[1]) - (p1[1] - ctr[1]) * (p2[0] - ctr[0]));
        vol6 += d;
        avol6 += std::fabs(d);
        tri_vol[t] = d;
        comp[find(a)] = find(bb);
        comp[find(bb)] = find(c3);
    }
    if (ok) {
        std::map<int, std::pair<double, double>> shell;   // root -> (signed, absolute) volume * 6
        for (int t = 0; t < nt; ++t) {
            if (tri_vol[t] == 0.0) continue;
            auto& sv = shell[find(wid[T[3 * t]])];
            sv.first += tri_vol[t];
            sv.second += std::fabs(tri_vol[t]);
        }
        for (const auto& sv : shell)
            if (!(std::fabs(sv.second.first) > 1e-6 * sv.second.second) || (sv.second.first > 0.0) != (vol6 > 0.0)) ok = false;
    }
    if (ok)
        for (const auto& e : edges)
            if (edges.find({e.first.second, e.first.first}) == edges.end()) { ok = false; break; }
    if (ok && !edges.empty() && std::fabs(vol6) > 1e-6 * avol6) return vol6 > 0.0 ? 1 : -1;
    return 0;
}

// Cluster order: recursive median bisection of the triangles in (centroid / extent,
// 0.5 * unit normal) space, always along the widest of the six axes, left halves a whole
// number of 64-triangle clusters.  Every aligned run of 64 is then a compact surface
// patch with a narrow normal cone (a plain Morton order of the centroids mixes the two
// sides of thin parts and gives cones too wide to cull by).  Returns the triangles in that order.
static inline std::vector<int> cluster_order(const double* V, const int32_t* T, int nt, const double lo[3], const double hi[3])
{
    const double ext = std::fmax(std::fmax(hi[0] - lo[0], hi[1] - lo[1]), std::fmax(hi[2] - lo[2], 1e-300));
    std::vector<std::array<double, 6>> feat(nt);
    for (int t = 0; t < nt; ++t) {
        const double* p0 = V + 3 * T[3 * t]; const double* p1 = V + 3 * T[3 * t + 1]; const double* p2 = V + 3 * T[3 * t + 2];
        double n3[3];
        const double len = tri_normal(p0, p1, p2, n3);
        for (int c3 = 0; c3 < 3; ++c3) {
            feat[t][c3] = (p0[c3] + p1[c3] + p2[c3]) / (3.0 * ext);
            feat[t][3 + c3] = len > 0.0 ? 0.5 * n3[c3] / len : 0.0;
        }
    }
    std::vector<int> idx(nt);
    for (int t = 0; t < nt; ++t) idx[t] = t;
    std::vector<std::pair<int, int>> stack;   // [begin, end) ranges still to split
    stack.push_back({0, nt});
    while (!stack.empty()) {
        const auto rg = stack.back();
        stack.pop_back();
        const int cnt = rg.second - rg.first;
        if (cnt <= 64) continue;
        int dim = 0;
        double best = -1.0;
        for (int d = 0; d < 6; ++d) {
            double mn = 1e300, mx = -1e300;
            for (int i = rg.first; i < rg.second; ++i) { mn = std::fmin(mn, feat[idx[i]][d]); mx = std::fmax(mx, feat[idx[i]][d]); }
            if (mx - mn > best) { best = mx - mn; dim = d; }
        }
        std::stable_sort(idx.begin() + rg.first, idx.begin() + rg.second,
                         [&](int x, int y) { return feat[x][dim] < feat[y][dim]; });
        const int left = ((cnt + 63) / 64 / 2) * 64;
        stack.push_back({rg.first, rg.first + left});
        stack.push_back({rg.first + left, rg.second});
    }
    return idx;
}

// vertex sharing: the unique vertices (by index) of every cluster of 64 and, per triangle, where
// its three sit in that list; a cluster with more than 64 of them is set up per triangle
static inline void share_cluster_vertices(const double* V, const int32_t* T, const std::vector<int>& order, size_t base, size_t end, PreparedMesh* m)
{
    const size_t nt = order.size();
    for (size_t c = base / 64; c < end / 64; ++c) {
        const size_t j0 = c * 64 - base, j1 = std::min<size_t>(j0 + 64, nt);
        std::map<int, int> local;
        bool fits = true;
        for (size_t j = j0; j < j1 && fits; ++j)
            for (int k = 0; k < 3; ++k) {
                const int vi = T[3 * order[j] + k];
                if (local.find(vi) == local.end()) {
                    if (local.size() == 64) { fits = false; break; }
                    const int pos = (int)local.size();
                    local[vi] = pos;
                    for (int c3 = 0; c3 < 3; ++c3) m->cluster_vtx[c * 192 + 64 * c3 + pos] = V[3 * vi + c3];
                }
            }
        if (!fits || local.empty()) continue;
        m->cluster_nv[c] = (int)local.size();
        for (size_t j = j0; j < j1; ++j) {
            unsigned pk = 0;
            for (int k = 0; k < 3; ++k) pk |= (unsigned)local[T[3 * order[j] + k]] << (8 * k);
            m->tri_local[base + j] = pk;
        }
    }
}

// model-space plane of each triangle, unit normal of its winding (float32 pre-cull only)
static inline void triangle_planes(size_t base, int nt, PreparedMesh* m)
{
    for (int j = 0; j < nt; ++j) {
        double p[3][3], n3[3];
        soup_triangle(*m, base + j, p);
        const double len = tri_normal(p[0], p[1], p[2], n3);
        if (!(len > 0.0) || !std::isfinite(len)) continue;   // zero area: stays NaN = kept (the setup rejects it)
        // offset from the triangle's centroid (the three vertices give the same plane up to rounding)
        const double cx3 = (p[0][0] + p[1][0] + p[2][0]) / 3.0, cy3 = (p[0][1] + p[1][1] + p[2][1]) / 3.0,
                     cz3 = (p[0][2] + p[1][2] + p[2][2]) / 3.0;
        float* pl = &m->tri_plane[4 * (base + j)];
        pl[0] = (float)(n3[0] / len); pl[1] = (float)(n3[1] / len); pl[2] = (float)(n3[2] / len);
        pl[3] = (float)(-(n3[0] * cx3 + n3[1] * cy3 + n3[2] * cz3) / len);
    }
}

// bounding sphere of each cluster of 64 (centre = bbox centre of its vertices) and, for a body that is
// culled (cull = +1 / -1), the cone of the cluster's outward unit normals
static inline void cluster_spheres_and_cones(size_t base, size_t end, size_t nt, int cull, PreparedMesh* m)
{
    const std::vector<double>& soup = m->soup;
    const size_t n_alloc = m->n_alloc;
    for (size_t c = base / 64; c < end / 64; ++c) {
        double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
        const size_t j0 = c * 64 - base, j1 = std::min<size_t>(j0 + 64, nt);
        for (size_t j = j0; j < j1; ++j)
            for (int k = 0; k < 3; ++k)
                for (int c3 = 0; c3 < 3; ++c3) {
                    const double x = soup[(size_t)(3 * k + c3) * n_alloc + base + j];
                    clo[c3] = std::fmin(clo[c3], x); chi[c3] = std::fmax(chi[c3], x);
                }
        double cc[3] = {0.5 * (clo[0] + chi[0]), 0.5 * (clo[1] + chi[1]), 0.5 * (clo[2] + chi[2])}, cr2 = 0.0;
        for (size_t j = j0; j < j1; ++j)
            for (int k = 0; k < 3; ++k) {
                double d2 = 0.0;
                for (int c3 = 0; c3 < 3; ++c3) {
                    const double d = soup[(size_t)(3 * k + c3) * n_alloc + base + j] - cc[c3];
                    d2 += d * d;
                }
                cr2 = std::fmax(cr2, d2);
            }
        for (int c3 = 0; c3 < 3; ++c3) m->cluster_sphere[4 * c + c3] = (float)cc[c3];
        m->cluster_sphere[4 * c + 3] = (float)(std::sqrt(cr2) * 1.0001 + 1e-6);
        if (cull != 0) {   // cone of the cluster's outward unit normals
            std::vector<std::array<double, 3>> nrm;
            double ax[3] = {0, 0, 0};
            for (size_t j = j0; j < j1; ++j) {
                double p[3][3], n3[3];
                soup_triangle(*m, base + j, p);
                const double len = tri_normal(p[0], p[1], p[2], n3);
                if (!(len > 0.0)) continue;   // zero area: never rendered
                for (int c3 = 0; c3 < 3; ++c3) { n3[c3] *= (double)cull / len; ax[c3] += n3[c3]; }
                nrm.push_back({n3[0], n3[1], n3[2]});
            }
            const double al = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            if (al > 1e-9 && !nrm.empty()) {
                double mindp = 1.0;
                for (const auto& n3 : nrm) mindp = std::fmin(mindp, (n3[0] * ax[0] + n3[1] * ax[1] + n3[2] * ax[2]) / al);
                for (int c3 = 0; c3 < 3; ++c3) m->cluster_cone[4 * c + c3] = (float)(ax[c3] / al);
                m->cluster_cone[4 * c + 3] = (float)(mindp - 1e-4);   // <= 0: the cone is too wide to cull by
            }
        }
    }
}

}  // namespace mesh_detail

// triangle soup (SoA) + bounding spheres.  Per body the triangles are ordered along a
// bisection of positions and normals and padded to a multiple of 64 with NaN triangles, so
// that every aligned run of 64 is a compact surface patch ("cluster") one wave rasterizes.
// allow_cull = false: no body is culled, whatever its surface.  Returns kMeshOk, or the error
// code with the message in *err (out is then unspecified).
static inline int prepare_mesh(const MeshInput& in, bool allow_cull, PreparedMesh* out, std::string* err)
{
    using namespace mesh_detail;
    long n_tri = 0;
    out->tri_begin[0] = 0;
    out->max_clusters = 0;
    for (int b = 0; b < in.n_bodies; ++b) {
        if (in.vertex_counts[b] <= 0 || in.triangle_counts[b] < 0)
            return fail(err, fmt("object %d: bad mesh counts", b));
        n_tri += ((long)in.triangle_counts[b] + 63) / 64 * 64;
        out->tri_begin[b + 1] = (int)n_tri;
        out->max_clusters = std::max(out->max_clusters, (out->tri_begin[b + 1] - out->tri_begin[b]) >> 6);
    }
    for (int b = in.n_bodies; b < kMeshMaxBodies; ++b) out->tri_begin[b + 1] = (int)n_tri;
    for (int b = 0; b < kMeshMaxBodies; ++b) out->tri_end[b] = out->tri_begin[b];
    if (n_tri > (1L << 30)) return fail(err, "too many triangles");
    const size_t n_alloc = (size_t)(n_tri > 0 ? n_tri : 64);
    out->n_alloc = n_alloc;
    out->soup.assign((size_t)9 * n_alloc, std::nan(""));
    out->cluster_sphere.assign(4 * (n_alloc / 64), 0.f);
    out->cluster_cone.assign(4 * (n_alloc / 64), -2.f);   // min cos -2: never culled
    out->tri_plane.assign(4 * n_alloc, std::nanf(""));    // NaN: never pre-culled
    out->cluster_vtx.assign((size_t)192 * (n_alloc / 64), 0.0);
    out->cluster_nv.assign(n_alloc / 64, 0);
    out->tri_local.assign(n_alloc, 0xffffffffu);
    size_t voff = 0, toff = 0;
    for (int b = 0; b < in.n_bodies; ++b) {
        const int nv = in.vertex_counts[b], nt = in.triangle_counts[b];
        const double* V = in.vertices + 3 * voff;
        const int32_t* T = in.triangles + 3 * toff;
        double lo[3] = {V[0], V[1], V[2]}, hi[3] = {V[0], V[1], V[2]};
        for (int i = 0; i < nv; ++i)
            for (int c3 = 0; c3 < 3; ++c3) {
                const double x = V[3 * i + c3];
                if (!std::isfinite(x))
                    return fail(err, fmt("object %d: non-finite vertex", b));
                lo[c3] = std::fmin(lo[c3], x);
                hi[c3] = std::fmax(hi[c3], x);
            }
        double ctr[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
        double r2 = 0.0;
        for (int i = 0; i < nv; ++i) {
            const double dx = V[3 * i] - ctr[0], dy = V[3 * i + 1] - ctr[1], dz = V[3 * i + 2] - ctr[2];
            r2 = std::fmax(r2, dx * dx + dy * dy + dz * dz);
        }
        out->sphere[b][0] = ctr[0]; out->sphere[b][1] = ctr[1]; out->sphere[b][2] = ctr[2];
        out->sphere[b][3] = std::sqrt(r2) * (1.0 + 1e-9) + 1e-12;
        for (int t = 0; t < nt; ++t)
            for (int k = 0; k < 3; ++k)
                if (T[3 * t + k] < 0 || T[3 * t + k] >= nv)
                    return fail(err, fmt("object %d triangle %d: vertex index %d out of range", b, t, T[3 * t + k]));
        out->body_cull[b] = allow_cull && nt >= 4 ? closed_surface_sign(V, nv, T, nt, ctr) : 0;
        const std::vector<int> order = cluster_order(V, T, nt, lo, hi);
        const size_t base = (size_t)out->tri_begin[b], end = (size_t)out->tri_begin[b + 1];
        for (int j = 0; j < nt; ++j) {
            const int t = order[j];
            for (int k = 0; k < 3; ++k)
                for (int c3 = 0; c3 < 3; ++c3)
                    out->soup[(size_t)(3 * k + c3) * n_alloc + base + j] = V[3 * T[3 * t + k] + c3];
        }
        out->tri_end[b] = (int)base + nt;
        share_cluster_vertices(V, T, order, base, end, out);
        triangle_planes(base, nt, out);
        cluster_spheres_and_cones(base, end, (size_t)nt, out->body_cull[b], out);
        voff += nv;
        toff += nt;
    }
    // float32 copy of the vertices, per body (screen rectangles)
    out->vtx.clear();
    size_t vo = 0;
    out->vtx_begin[0] = 0;
    for (int b = 0; b < in.n_bodies; ++b) {
        for (int i = 0; i < in.vertex_counts[b]; ++i) {
            for (int c3 = 0; c3 < 3; ++c3) out->vtx.push_back((float)in.vertices[3 * (vo + i) + c3]);
            out->vtx.push_back(0.f);
        }
        vo += (size_t)in.vertex_counts[b];
        out->vtx_begin[b + 1] = (int)vo;
    }
    for (int b = in.n_bodies; b < kMeshMaxBodies; ++b) out->vtx_begin[b + 1] = (int)vo;
    return kMeshOk;
}

}  // namespace rbs
