// Stand-alone driver of rbs::prepare_mesh (dbot_ros_amd/csrc/rbs_mesh.h) for tests/test_mesh_prep_cpu.py: no GPU, no HIP.
//
//   mesh_prep_check <input> <arrays out> [nocull]
//
// input (binary, native endianness): int32 n_bodies, int32 vertex_counts[n_bodies], int32 triangle_counts[n_bodies],
// float64 vertices[3 * sum of the positive vertex counts], int32 triangles[3 * sum of the positive triangle counts].
// stdout: "rc <code>", then either "err <message>" or the scalar results and one "array <name> <type> <count>" line per
// output array; the arrays themselves follow one another, raw, in that order in <arrays out>.
// Exit status 0 whenever prepare_mesh was called and answered (also with an error code); 2: bad usage or input file.
#include "../../dbot_ros_amd/csrc/rbs_mesh.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

template <class T>
bool read_n(FILE* f, std::vector<T>* v, size_t n)
{
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

template <class T>
bool write_array(FILE* f, const char* name, const char* type, const std::vector<T>& v)
{
    printf("array %s %s %zu\n", name, type, v.size());
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

void print_ints(const char* name, const int* v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %d", v[i]);
    printf("\n");
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3 || argc > 4 || (argc == 4 && std::strcmp(argv[3], "nocull"))) {
        fprintf(stderr, "usage: %s <input> <arrays out> [nocull]\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t nb = 0;
    std::vector<int32_t> vc, tc, tris;
    std::vector<double> verts;
    bool ok = fread(&nb, sizeof nb, 1, f) == 1 && nb >= 1 && nb <= rbs::kMeshMaxBodies;
    ok = ok && read_n(f, &vc, (size_t)nb) && read_n(f, &tc, (size_t)nb);
    size_t nv = 0, nt = 0;
    if (ok)
        for (int b = 0; b < nb; ++b) { nv += vc[b] > 0 ? (size_t)vc[b] : 0; nt += tc[b] > 0 ? (size_t)tc[b] : 0; }
    ok = ok && read_n(f, &verts, 3 * nv) && read_n(f, &tris, 3 * nt) && fgetc(f) == EOF;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a mesh set\n", argv[1]); return 2; }

    const rbs::MeshInput in = {nb, verts.data(), vc.data(), tris.data(), tc.data()};
    rbs::PreparedMesh m;
    std::string err;
    const int rc = rbs::prepare_mesh(in, argc != 4, &m, &err);
    printf("rc %d\n", rc);
    if (rc != rbs::kMeshOk) {
        printf("err %s\n", err.c_str());
        return 0;
    }
    printf("n_alloc %zu\nmax_clusters %d\n", m.n_alloc, m.max_clusters);
    print_ints("tri_begin", m.tri_begin, rbs::kMeshMaxBodies + 1);
    print_ints("tri_end", m.tri_end, rbs::kMeshMaxBodies);
    print_ints("vtx_begin", m.vtx_begin, rbs::kMeshMaxBodies + 1);
    print_ints("body_cull", m.body_cull, nb);
    for (int b = 0; b < nb; ++b) printf("sphere %d %a %a %a %a\n", b, m.sphere[b][0], m.sphere[b][1], m.sphere[b][2], m.sphere[b][3]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    ok = write_array(o, "soup", "f64", m.soup) && write_array(o, "cluster_sphere", "f32", m.cluster_sphere) &&
         write_array(o, "cluster_cone", "f32", m.cluster_cone) && write_array(o, "tri_plane", "f32", m.tri_plane) &&
         write_array(o, "cluster_vtx", "f64", m.cluster_vtx) && write_array(o, "cluster_nv", "i32", m.cluster_nv) &&
         write_array(o, "tri_local", "u32", m.tri_local) && write_array(o, "vtx", "f32", m.vtx);
    ok = (fclose(o) == 0) && ok;
    if (!ok) { fprintf(stderr, "%s: write failed\n", argv[2]); return 2; }
    return 0;
}
