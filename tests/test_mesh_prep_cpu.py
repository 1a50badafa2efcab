"""The mesh preparation (dbot_ros_amd/csrc/rbs_mesh.h: what sensor creation turns the caller's meshes into before the
raster kernels see them) checked WITHOUT a GPU.  tests/cpp/mesh_prep_check.cpp is a stand-alone program around
rbs::prepare_mesh; it is built twice, plainly and under ASan + UBSan, and both are run as child processes.

  * Every output is held BIT FOR BIT to tests/golden/mesh_prep.json, which was recorded from the code as it stood inside
    create_impl before the header existed (provenance in the file).  The file also holds the sha256 of every input, so that a
    drift of the mesh generators shows as an input mismatch and not as a preparation failure.
  * The culling decision (DevParams::body_cull) is asserted outright: the GPU culling tests only show that culling never
    changes a depth, and would pass if a closed mesh silently stopped being culled.
  * The structure the kernels rely on is recomputed in numpy from the outputs.
  * The validation errors, with their messages.
"""
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import mesh_cases
from dbot_ros_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
GOLDEN = os.path.join(HERE, "golden", "mesh_prep.json")
DTYPES = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "u32": np.uint32}
MAX_BODIES = 16
# the cone of a cluster that is never culled: the kernels read "min cos <= -1".  The parent's code fills all four floats with
# -2 (not an axis of zeros and -2), and every output is held to the parent's: that is what is asserted
UNCULLED_CONE = -2.0


def _strip(n_tri):
    """A zigzag strip of n_tri triangles, consistently wound, not closed."""
    k = np.arange(n_tri + 2)
    v = np.stack([0.005 * k, 0.01 * (k % 2), 0.002 * (k % 3)], -1)
    t = np.array([(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(n_tri)], np.int32).reshape(-1, 3)
    return v, t


@functools.lru_cache(maxsize=None)
def cases():
    """name -> list of bodies (vertices float64 [nv][3], triangles int32 [nt][3]): the meshes that must prepare."""
    out = {}
    for name, m in mesh_cases.mesh_variants().items():
        out["m1_" + name] = [m]
    for name in mesh_cases.VARIANTS:
        out["box_" + name] = [mesh_cases.box_variant(name)]
    out["two_bodies"] = [synth.mesh_m1(level=2), synth.mesh_box12()]
    out["m4"] = [synth.mesh_m4()]                               # 795 clusters: more than the shared-cull kernels take
    three = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]])
    out["no_triangles"] = [(three, np.zeros((0, 3), np.int32))]
    out["one_triangle"] = [(three, np.array([[0, 1, 2]], np.int32))]
    out["tri64"] = [_strip(64)]                                 # exactly one cluster, no padding
    out["tri65"] = [_strip(65)]                                 # one triangle in the second cluster
    out["tri62"] = [_strip(62)]                                 # 64 distinct vertices in the cluster: the most that are shared
    out["tri63"] = [_strip(63)]                                 # 65: one too many, the cluster is set up per triangle
    v, t = mesh_cases.mesh_variants()["closed"]
    out["m1_doubled"] = [(v, np.concatenate([t, t]))]           # every directed edge twice: not a surface, never culled
    v, t = mesh_cases.box(0.0, 64 / 256, -16 / 256, 32 / 256, 1.0, 2.0)
    v = v[t]                                                    # unwelded, and every other triangle spells its zeros -0.0
    v[1::2][v[1::2] == 0.0] = -0.0
    out["box_signed_zeros"] = [(v.reshape(-1, 3), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3))]
    return {k: [(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(t, np.int32).reshape(-1, 3)) for v, t in bodies]
            for k, bodies in out.items()}


# what body_cull must be (the issue's table); every body of every other case has fewer than 4 triangles or is open: 0
CULL = {"closed": 1, "unwelded": 1, "two_shells": 1, "closed_inward": -1, "with_holes": 0, "mixed_winding": 0, "one_shell_inside_out": 0}


def _raw(bodies):
    return ([len(v) for v, _ in bodies], [len(t) for _, t in bodies],
            np.concatenate([v.reshape(-1) for v, _ in bodies]), np.concatenate([t.reshape(-1) for _, t in bodies]))


@functools.lru_cache(maxsize=None)
def error_cases():
    """name -> ((vertex counts, triangle counts, vertices, triangles), the message): the meshes that must be refused."""
    m1, box12 = cases()["two_bodies"]
    out = {}
    v = box12[0].copy()
    v[5, 1] = np.nan
    out["non_finite_vertex"] = (_raw([m1, (v, box12[1])]), "object 1: non-finite vertex")
    t = m1[1].copy()
    t[5, 2] = -1
    out["index_minus_one"] = (_raw([(m1[0], t)]), "object 0 triangle 5: vertex index -1 out of range")
    t = m1[1].copy()
    t[7, 0] = len(m1[0])
    out["index_is_vertex_count"] = (_raw([(m1[0], t)]), f"object 0 triangle 7: vertex index {len(m1[0])} out of range")
    out["no_vertices"] = (([0], [0], np.zeros(0), np.zeros(0, np.int32)), "object 0: bad mesh counts")
    vc, tc, vv, tt = _raw([m1, box12])
    out["negative_triangle_count"] = ((vc, [tc[0], -1], vv, tt[:3 * tc[0]]), "object 1: bad mesh counts")
    return out


def input_bytes(vc, tc, verts, tris):
    return b"".join([np.array([len(vc)], np.int32).tobytes(), np.asarray(vc, np.int32).tobytes(), np.asarray(tc, np.int32).tobytes(),
                     np.ascontiguousarray(verts, np.float64).tobytes(), np.ascontiguousarray(tris, np.int32).tobytes()])


@functools.lru_cache(maxsize=None)
def all_inputs():
    """name -> the input file's bytes, for the good and the refused meshes alike."""
    out = {name: input_bytes(*_raw(bodies)) for name, bodies in cases().items()}
    out.update({name: input_bytes(*raw) for name, (raw, _) in error_cases().items()})
    return out


def run_check(exe, blob, workdir, nocull=False):
    """One run of a check program: (return code, stderr, {"rc", "err" | "scalars" (text lines), "arrays" (name -> numpy)})."""
    os.makedirs(workdir, exist_ok=True)
    src, dst = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, src, dst] + (["nocull"] if nocull else []), capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    res = {"rc": int(lines[0].split()[1]) if lines and lines[0].startswith("rc ") else None}
    if res["rc"] == 0:
        res["scalars"] = [ln for ln in lines[1:] if not ln.startswith("array ")]
        res["arrays"] = {}
        with open(dst, "rb") as f:
            for ln in lines:
                if ln.startswith("array "):
                    _, name, typ, count = ln.split()
                    res["arrays"][name] = np.frombuffer(f.read(int(count) * np.dtype(DTYPES[typ]).itemsize), DTYPES[typ])
                    assert res["arrays"][name].size == int(count), name
            assert f.read() == b""
    elif res["rc"] is not None:
        res["err"] = lines[1][len("err "):]
    return r.returncode, r.stderr, res


def digest(res):
    """What the golden file keeps of a run."""
    if res["rc"] != 0:
        return {"rc": res["rc"], "err": res["err"]}
    return {"rc": 0, "scalars": res["scalars"], "arrays": {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in res["arrays"].items()}}


@pytest.fixture(scope="module")
def exes():
    subprocess.check_call(["make", "-s", "-C", CPP, "mesh_prep_check", "mesh_prep_check_san"])
    return {"plain": os.path.join(CPP, "mesh_prep_check"), "san": os.path.join(CPP, "mesh_prep_check_san")}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def prepared(exes, tmp_path_factory):
    """(case, build, nocull) -> the run's result, each computed once."""
    inputs, tmp, memo = all_inputs(), tmp_path_factory.mktemp("mesh_prep"), {}

    def get(name, build="plain", nocull=False):
        key = (name, build, nocull)
        if key not in memo:
            code, stderr, res = run_check(exes[build], inputs[name], str(tmp), nocull)
            assert code == 0 and stderr == "", (key, code, stderr[-2000:])
            memo[key] = res
        return memo[key]
    return get


def _scalars(res):
    s = {ln.split()[0]: ln.split()[1:] for ln in res["scalars"] if not ln.startswith("sphere ")}
    out = {k: np.array(v, np.int64) for k, v in s.items()}
    out["sphere"] = np.array([[float.fromhex(x) for x in ln.split()[2:]] for ln in res["scalars"] if ln.startswith("sphere ")])
    return out


@pytest.mark.parametrize("name", sorted(all_inputs()))
def test_inputs_are_the_recorded_ones(golden, name):
    assert hashlib.sha256(all_inputs()[name]).hexdigest() == golden["cases"][name]["input_sha256"]


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("name", sorted(all_inputs()))
def test_outputs_are_the_parents_bit_for_bit(prepared, golden, name, build):
    """Both builds, with and without culling allowed: the scalar results and every array's sha256 are the recorded ones
    (the sanitizer build also exits 0 with nothing on stderr: `prepared` asserts that of every run)."""
    for nocull in (False, True):
        assert digest(prepared(name, build, nocull)) == golden["cases"][name]["nocull" if nocull else "cull"], (name, build, nocull)


def test_the_culling_decision(prepared):
    """Closed and consistently wound, also unwelded or in several shells: culled, with the sign of the winding.  Holes, mixed
    winding, one shell inside out, fewer than 4 triangles: never.  (Observed on the parent for closed, inward, holes and
    unwelded M1: +1, -1, 0, +1.)"""
    for name, bodies in cases().items():
        cull = _scalars(prepared(name))["body_cull"]
        variant = name.split("_", 1)[1] if name.startswith(("m1_", "box_")) else None
        # (beyond the table: closed bodies are culled, -0.0 welds with 0.0, a surface listed twice is no surface)
        want = [CULL[variant]] if variant in CULL else {"two_bodies": [1, 1], "m4": [1], "box_signed_zeros": [1]}.get(name, [0])
        assert cull.tolist() == want, (name, cull.tolist(), want)
        for (v, t), c in zip(bodies, cull):
            if len(t) < 4:
                assert c == 0, name
        assert not _scalars(prepared(name, nocull=True))["body_cull"].any(), name


@pytest.mark.parametrize("name", sorted(cases()))
def test_allow_cull_changes_the_cones_alone(prepared, name):
    a, b = prepared(name), prepared(name, nocull=True)
    for k in a["arrays"]:
        if k != "cluster_cone":
            assert np.array_equal(a["arrays"][k].view(np.uint8), b["arrays"][k].view(np.uint8)), k
    assert np.array_equal(b["arrays"]["cluster_cone"].reshape(-1, 4), np.full((b["arrays"]["cluster_nv"].size, 4), UNCULLED_CONE, np.float32))
    assert [ln for ln in a["scalars"] if not ln.startswith("body_cull")] == [ln for ln in b["scalars"] if not ln.startswith("body_cull")]


def _bits(rows):
    """Rows of doubles as sortable, exactly comparable tuples of their bit patterns."""
    return sorted(map(tuple, np.ascontiguousarray(rows, np.float64).view(np.uint64).tolist()))


@pytest.mark.parametrize("name", sorted(cases()))
def test_structure_the_kernels_rely_on(prepared, name):
    bodies = cases()[name]
    res = prepared(name)
    S, A = _scalars(res), res["arrays"]
    nb, n_alloc = len(bodies), int(S["n_alloc"][0])
    tb, te, vb = S["tri_begin"], S["tri_end"], S["vtx_begin"]
    assert n_alloc % 64 == 0 and n_alloc == max(64, sum((len(t) + 63) // 64 * 64 for _, t in bodies))
    assert int(S["max_clusters"][0]) == max((len(t) + 63) // 64 for _, t in bodies)
    assert tb.size == MAX_BODIES + 1 and (tb % 64 == 0).all() and (tb[nb:] == tb[nb]).all() and (te[nb:] == tb[nb:-1]).all()
    assert vb.tolist() == np.concatenate([[0], np.cumsum([len(v) for v, _ in bodies]), [sum(len(v) for v, _ in bodies)] * (MAX_BODIES - nb)]).tolist()
    soup = A["soup"].reshape(9, n_alloc)
    tri = soup.T.reshape(n_alloc, 3, 3)                         # [triangle][vertex][coordinate]
    plane, local = A["tri_plane"].reshape(n_alloc, 4), A["tri_local"]
    sphere, cone = A["cluster_sphere"].reshape(-1, 4).astype(np.float64), A["cluster_cone"].reshape(-1, 4)
    cvtx, cnv = A["cluster_vtx"].reshape(-1, 3, 64), A["cluster_nv"]
    assert len(sphere) == len(cone) == len(cvtx) == len(cnv) == n_alloc // 64 and local.size == n_alloc
    pad = np.ones(n_alloc, bool)
    vtx32 = A["vtx"].reshape(-1, 4)
    for b, (v, t) in enumerate(bodies):
        assert te[b] == tb[b] + len(t) and tb[b + 1] == tb[b] + (len(t) + 63) // 64 * 64
        pad[tb[b]:te[b]] = False
        # the float32 vertex copy, and the body's sphere around every vertex
        assert np.array_equal(vtx32[vb[b]:vb[b + 1]], np.concatenate([v.astype(np.float32), np.zeros((len(v), 1), np.float32)], 1))
        assert (np.linalg.norm(v - S["sphere"][b, :3], axis=1) <= S["sphere"][b, 3]).all()
        # the soup's triangles: a permutation of the input's
        mine = tri[tb[b]:te[b]].reshape(-1, 9)
        assert _bits(mine) == _bits(v[t].reshape(-1, 9))
        # which input triangle each one is (equal triangles in any order), hence the vertex indices of every cluster
        where = {}
        for i, row in enumerate(map(tuple, v[t].reshape(-1, 9).view(np.uint64).tolist())):
            where.setdefault(row, []).append(i)
        order = np.array([where[row].pop() for row in map(tuple, np.ascontiguousarray(mine).view(np.uint64).tolist())], np.int64)
        cull = int(S["body_cull"][b])
        for c in range(tb[b] // 64, tb[b + 1] // 64):
            j0, j1 = c * 64, min(c * 64 + 64, int(te[b]))
            idx = t[order[j0 - tb[b]:j1 - tb[b]]]
            distinct = len(set(idx.reshape(-1).tolist()))
            # vertex sharing: at most 64 distinct vertex indices, else the cluster is set up per triangle
            assert cnv[c] == (distinct if distinct <= 64 else 0), (name, c, distinct, cnv[c])
            if cnv[c]:
                pk = local[j0:j1]
                assert (pk >> 24 == 0).all()
                for k in range(3):
                    pos = (pk >> (8 * k)) & 0xff
                    assert (pos < cnv[c]).all()
                    assert np.array_equal(np.ascontiguousarray(cvtx[c][:, pos].T).view(np.uint64), np.ascontiguousarray(tri[j0:j1, k]).view(np.uint64))
            else:
                assert (local[j0:j1] == 0xffffffff).all()
            # the cluster's sphere holds its vertices
            assert (np.linalg.norm(tri[j0:j1].reshape(-1, 3) - sphere[c, :3], axis=1) <= sphere[c, 3]).all()
            # its cone holds the outward normal of every triangle with an area
            if cull == 0:
                assert cone[c].tolist() == [UNCULLED_CONE] * 4
            else:
                n3 = np.cross(tri[j0:j1, 1] - tri[j0:j1, 0], tri[j0:j1, 2] - tri[j0:j1, 0])
                ln = np.linalg.norm(n3, axis=1)
                unit = cull * n3[ln > 0] / ln[ln > 0, None]
                assert (unit @ cone[c, :3].astype(np.float64) >= float(cone[c, 3])).all(), (name, c)
        # the planes: unit normal of the winding through the triangle (float32: 1e-6), NaN for a triangle without area
        n3 = np.cross(tri[tb[b]:te[b], 1] - tri[tb[b]:te[b], 0], tri[tb[b]:te[b], 2] - tri[tb[b]:te[b], 0])
        ln = np.linalg.norm(n3, axis=1)
        pl = plane[tb[b]:te[b]].astype(np.float64)
        assert np.isnan(pl[ln == 0]).all()
        ok = ln > 0
        assert np.abs(pl[ok, :3] - n3[ok] / ln[ok, None]).max(initial=0) <= 1e-6
        assert np.abs((tri[tb[b]:te[b]][ok] * pl[ok, None, :3]).sum(-1) + pl[ok, None, 3]).max(initial=0) <= 1e-6
    # padding: NaN triangles, NaN planes, no local indices
    assert pad.sum() == n_alloc - sum(len(t) for _, t in bodies)
    assert np.isnan(soup[:, pad]).all() and np.isnan(plane[pad]).all() and (local[pad] == 0xffffffff).all()
    if name == "m1_unwelded":
        assert (cnv == 0).all()                                 # 192 distinct indices in every full cluster
    if name == "m1_closed":
        assert (cnv > 0).all()


@pytest.mark.parametrize("build", ["plain", "san"])
@pytest.mark.parametrize("name", sorted(error_cases()))
def test_bad_meshes_are_refused_with_their_message(prepared, name, build):
    for nocull in (False, True):
        res = prepared(name, build, nocull)
        assert res["rc"] == -1 and res["err"] == error_cases()[name][1], res
