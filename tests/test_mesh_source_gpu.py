"""hk_add_meshes_device: meshes whose arrays lie in device memory.  The builder declares them by their counts, the call assembles their
HkPrimitive / HkVertex records on the device (k_assemble_meshes) and gives the geometry back to the builder; afterwards the context, the
builder and the mirrors must hold, byte for byte, what hk_add_meshes leaves for a twin that got the same values from host arrays - here
checked against a fresh context that uploaded the twin builder (add_mesh + rebuild_mesh_tree), as tests/test_add_meshes_gpu.py does.
Every case runs with the product's default traversal (8 orderings) and under the suite's HK_CTX_EXACT_TRAVERSAL.  Byte equality
throughout: no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd._ffi import HikariError
from bevy_hikari_amd.plugin import mesh_sources_device
from cases import diff_buffers, snapshot
from test_add_meshes_gpu import MODES, base_builder, geometry_equal, place, plugin, view
from test_mesh_deform_gpu import SETTINGS
from test_mesh_rebuild_gpu import SIZED, soup
from test_scene_load_gpu import assert_builders_equal, nodes_equal, render_and_compare

pytestmark = pytest.mark.gpu

LIST, STRIP = F.TOPOLOGY_TRIANGLE_LIST, F.TOPOLOGY_TRIANGLE_STRIP
RECORD_BYTES = lambda spec: 48 * triangles(spec) + 32 * len(spec["p"])


def torch_():
    import torch

    return torch


def spec(positions, indices, topology=LIST, seed=0, uvs=True):
    """one mesh: positions, unit normals and uvs that differ per vertex (so that a misplaced one shows), indices or None"""
    rng = np.random.default_rng(1000 + seed + len(positions))
    n = rng.normal(size=(len(positions), 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    uv = rng.uniform(0.0, 1.0, (len(positions), 2)).astype(np.float32) if uvs else None
    return dict(p=np.ascontiguousarray(positions, np.float32), n=n, uv=uv, i=None if indices is None else np.ascontiguousarray(indices, np.uint32), topology=topology)


def triangles(s):
    n = len(s["p"]) if s["i"] is None else len(s["i"])
    return n // 3 if s["topology"] == LIST else n - 2


def sized(name):
    return spec(SIZED[name][0], SIZED[name][2])


def of_soup(k, seed, **kw):
    p, _, i = soup(k, seed)
    return spec(p, i, seed=seed, **kw)


def five_vertices():
    p = np.array([[0, 0, 0], [0.4, 0, 0], [0, 0.4, 0], [3, -2, 5], [0.4, 0.4, 0]], np.float32)   # vertex 3: unused, outside the triangles' box
    return spec(p, [0, 1, 2, 2, 1, 4])


def strip(n_triangles, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.3, 0.3, (n_triangles + 4, 3)).astype(np.float32)
    return spec(p, rng.permutation(len(p))[:n_triangles + 2], STRIP, seed)


def declare(b, s):
    return b.declare_mesh(len(s["p"]), 0 if s["i"] is None else len(s["i"]), s["topology"])


def twin_add(b, s, deferred=True):
    """what the twin builder holds: the same values from host arrays, the tree of hk_scene_builder_rebuild_mesh_tree where the device builds one"""
    uv = s["uv"] if s["uv"] is not None else np.zeros((len(s["p"]), 2), np.float32)
    m = b.add_mesh(s["p"], s["n"], uv, s["i"], s["topology"])
    if deferred:
        b.rebuild_mesh_tree(m)
    return m


def host_add(b, s, deferred):
    """a mesh the host adds to the device run's builder the ordinary way"""
    return b.add_mesh(s["p"], s["n"], s["uv"], s["i"], s["topology"], build_tree=not deferred)


def source(s, how="packed", device="cuda:0"):
    """the arrays of one mesh as torch tensors: packed, or ("sliced") positions and normals as column slices of one [n, 8] state tensor
    and the uvs at stride 16"""
    torch = torch_()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = dict(positions=dev(s["p"]), normals=dev(s["n"]))
    if how == "sliced":
        state = torch.full((len(s["p"]), 8), 7.5, device=device)
        state[:, 0:3] = out["positions"]
        state[:, 4:7] = out["normals"]
        out = dict(positions=state[:, 0:3], normals=state[:, 4:7])
    if s["uv"] is not None:
        out["uvs"] = dev(s["uv"])
        if how == "sliced":
            wide = torch.full((len(s["p"]), 4), -3.0, device=device)
            wide[:, 1:3] = out["uvs"]
            out["uvs"] = wide[:, 1:3]
    if s["i"] is not None:
        out["indices"] = dev(s["i"].view(np.int32))
    return out


def instance_all(gpu, twin, d, t, mat, ids):
    for b in (d, t):
        for k, m in enumerate(ids):
            b.add_instance(m, mat, place(k))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    twin.set_scene(t.finish())


# ---------------------------------------------------------------------------------------------------------------- 1. one call with everything
def everything():
    """(spec, kind) in builder order: device sources with the host's two meshes among them, so that the append sees several runs"""
    out = [(sized("1"), "device"), (sized("2"), "sliced"), (of_soup(255, 21), "device"), (of_soup(256, 22), "sliced"),
           (of_soup(300, 91), "host deferred"),
           (of_soup(257, 23, uvs=False), "device"), (sized("1023"), "device"), (sized("1024"), "sliced"), (sized("1025"), "device"),
           (spec(soup(7, 24)[0], None, seed=24), "device"), (strip(3, 25), "device"), (strip(4, 26), "sliced"),
           (spec(*S._sphere(6, 7)[0:4:3]), "host built"),
           (five_vertices(), "device"), (sized("half_split_40000"), "device")]
    return out


@MODES
def test_one_call_with_everything_equals_the_twin(threaded):
    torch = torch_()
    (d, mat, base_ids), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    _, _, orderings = gpu.engine.read_mesh_nodes()   # (lays the scene out)
    ids, sources, host_bytes, device_tris = [], {}, 0, 0
    for s, kind in everything():
        if kind.startswith("host"):
            ids.append(host_add(d, s, kind == "host deferred"))
            host_bytes += RECORD_BYTES(s)
        else:
            ids.append(declare(d, s))
            sources[ids[-1]] = source(s, "sliced" if kind == "sliced" else "packed")
            device_tris += triangles(s)
        assert twin_add(t, s, kind != "host built") == ids[-1]
    d.finish()
    t.finish()
    for m in ids:
        a, b = d.mesh_index(m), t.mesh_index(m)
        assert (a.vertex, a.primitive, a.node_offset, a.node_count) == (b.vertex, b.primitive, b.node_offset, b.node_count)
    assert d.unresolved_meshes() == len(sources) == 13 and d.pending_mesh_trees() == 14
    gpu.add_meshes(d, F.TREE_SAH, sources=sources)
    torch.cuda.synchronize()
    assert d.unresolved_meshes() == 0 and d.pending_mesh_trees() == 0
    assert_builders_equal(d, t, "after the add")
    taken = gpu.engine.last_add_sources()
    meshes, tris, launches, on_host, relocated = gpu.engine.last_add()
    print(f"add: {taken[0]} sources / {taken[1]} triangles assembled in {taken[2]} launch, {taken[3]} record bytes staged; {meshes} trees built in {launches} launches")
    assert taken == (13, device_tris, 1, host_bytes)
    assert (meshes, on_host, relocated) == (14, 1, 1)
    instance_all(gpu, twin, d, t, mat, ids)
    assert nodes_equal(gpu, twin, "everything")[1] == orderings == (8 if threaded else 1)
    geometry_equal(gpu, twin, t, base_ids + ids, "everything")
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "everything")
    # a second context given the completed builder through plain hk_add_meshes holds the same mesh level
    (again, _, _) = base_builder()
    second = plugin(threaded)
    second.set_scene(again.scene())
    second.engine.read_mesh_nodes()
    for s, kind in everything():
        twin_add(again, s, kind != "host built")
    again.finish()
    second.add_meshes(again)
    assert second.engine.last_add_sources()[:3] == (0, 0, 0)
    for k, m in enumerate(ids):
        again.add_instance(m, mat, place(k))
    second.engine.update_instances_on_device(again, F.TREE_SAH)
    nodes_equal(second, twin, "the second context")
    geometry_equal(second, twin, t, ids, "the second context")


# ---------------------------------------------------------------------------------------------------------------- 2. launches
@MODES
def test_forty_sources_take_the_launches_of_four(threaded):
    counts = {}
    for n in (40, 4):
        b, _, _ = base_builder()
        p = plugin(threaded)
        p.set_scene(b.scene())
        p.engine.read_mesh_nodes()   # (lays the scene out, as a frame would: the add then appends)
        sources = {}
        for k in range(n):
            s = of_soup(40, 500 + k)
            sources[declare(b, s)] = source(s)
        b.finish()
        p.add_meshes(b, sources=sources)
        counts[n] = (p.engine.last_add_sources(), p.engine.last_add())
        assert counts[n][0] == (n, 40 * n, 1, 0) and counts[n][1][0] == n and counts[n][1][3] == 0, counts[n]
    print(f"40 sources: {counts[40][0][2]} + {counts[40][1][2]} launches, 4 sources: {counts[4][0][2]} + {counts[4][1][2]}")
    assert counts[40][0][2] == counts[4][0][2] == 1 and counts[40][1][2] <= counts[4][1][2], counts


# ---------------------------------------------------------------------------------------------------------------- 3. a bad index
@pytest.mark.parametrize("bad", [None, 0xFFFFFFFF], ids=["n_vertices", "ffffffff"])
@MODES
def test_a_bad_index_writes_nothing(threaded, bad):
    """The kernel must survive the read: the index is never followed (vertex 0 is read instead), the source is flagged."""
    torch = torch_()
    (d, mat, _), (t, _, _), (plain, _, _) = base_builder(), base_builder(), base_builder()
    gpu, twin, control = plugin(threaded), plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    control.set_scene(plain.scene())
    cam, lights, s = view()
    render_and_compare([gpu, control], cam, s, lights, (1,), "before the call")
    specs = [of_soup(300, 31), five_vertices(), of_soup(513, 32)]
    ids = [declare(d, q) for q in specs]
    assert ids == [twin_add(t, q) for q in specs]
    d.finish()
    wrong = dict(specs[2], i=specs[2]["i"].copy())
    wrong["i"][-1] = len(wrong["p"]) if bad is None else bad      # the last corner of the last triangle of the last source
    before = bytes(gpu.engine.read_mesh_nodes()[0]), {n: bytes(getattr(d.scene(), n)) for n in ("vertices", "primitives", "asset_nodes", "instances")}
    with pytest.raises(HikariError) as refused:
        gpu.add_meshes(d, sources={ids[0]: source(specs[0]), ids[1]: source(specs[1]), ids[2]: source(wrong)})
    assert refused.value.code == F.HK_E_INVALID and "source 2" in str(refused.value), str(refused.value)
    assert d.unresolved_meshes() == 3 and d.pending_mesh_trees() == 3
    assert before == (bytes(gpu.engine.read_mesh_nodes()[0]), {n: bytes(getattr(d.scene(), n)) for n in before[1]})
    render_and_compare([gpu, control], cam, s, lights, (2,), "after the refusal")
    # ... and the same call with the index mended succeeds
    gpu.add_meshes(d, sources={m: source(q, "sliced") for m, q in zip(ids, specs)})
    torch.cuda.synchronize()
    t.finish()
    assert d.unresolved_meshes() == 0
    assert_builders_equal(d, t, "the same call with the index mended")
    instance_all(gpu, twin, d, t, mat, ids)
    nodes_equal(gpu, twin, "mended")
    geometry_equal(gpu, twin, t, ids, "mended")


# ---------------------------------------------------------------------------------------------------------------- 4. host-side refusals
@MODES
def test_host_side_refusals_write_nothing(threaded):
    """Every HK_E_INVALID of phase 0; the pointer cases rely on validation before any launch: nothing here may be made to fault."""
    torch = torch_()
    (d, mat, _), (plain, _, _) = base_builder(), base_builder()
    gpu, control = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    control.set_scene(plain.scene())
    api, e = gpu.engine.api, gpu.engine
    indexed, bare = of_soup(64, 41), spec(soup(9, 42)[0], None, seed=42)
    resolved = host_add(d, of_soup(20, 43), True)
    a, b = declare(d, indexed), declare(d, bare)
    d.finish()
    good = {a: source(indexed), b: source(bare)}
    host = np.zeros((len(indexed["p"]), 3), np.float32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
    block, size = C.c_void_p(), 1 << 21
    assert hip.hipMalloc(C.byref(block), size) == 0

    def table(n=2, **edits):
        """the good table with fields of entry 0 (mesh `a`, indexed) or - keys ending in 1 - entry 1 (mesh `b`, non-indexed) replaced"""
        tab, keep = mesh_sources_device(good, 0)
        for key, value in edits.items():
            entry, name = (tab[1], key[:-1]) if key.endswith("1") else (tab[0], key)
            setattr(entry, name, value)
        return tab, n, keep

    idx_ptr = good[a]["indices"].data_ptr()
    cases = {
        "a source naming a resolved mesh": table(mesh_id=resolved),
        "an unresolved mesh without a source": table(n=1),
        "a mesh named twice": table(mesh_id1=a),
        "an unknown mesh id": table(mesh_id=99),
        "indices given for a non-indexed declaration": table(indices1=idx_ptr),
        "no indices for an indexed declaration": table(indices=None),
        "no positions": table(positions=None),
        "no normals": table(normals1=None),
        "a misaligned pointer": table(positions=good[a]["positions"].data_ptr() + 2),
        "stride 10": table(normals_stride=10),
        "a stride below the packed size": table(uvs_stride=4),
        "a pageable host pointer": table(positions=host.ctypes.data),
        "an index array one element short of its allocation": table(indices=block.value + size - 4 * (len(indexed["i"]) - 1)),
        "positions one float short of their allocation": table(positions1=block.value + size - 12 * len(bare["p"]) + 4),
        "flags = 1": table(flags=1),
    }
    torch.cuda.synchronize()
    snap = lambda: (bytes(e.read_mesh_nodes()[0]), e.last_add(), e.last_add_sources(), d.unresolved_meshes(), d.pending_mesh_trees(), bytes(d.scene().primitives))
    before = snap()
    for what, (tab, n, keep) in cases.items():
        assert api.raw("add_meshes_device")(e.ctx, d.h, tab, n, F.TREE_SAH, None) == F.HK_E_INVALID, what
        assert api.last_error(), what
        assert snap() == before, what
    assert api.raw("add_meshes_device")(e.ctx, d.h, None, 2, F.TREE_SAH, None) == F.HK_E_INVALID
    assert api.raw("add_meshes_device")(e.ctx, d.h, table()[0], 2, 2, None) == F.HK_E_INVALID          # an unknown mode
    assert api.raw("add_meshes")(e.ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY and f"mesh {a}" in api.last_error()
    assert api.raw("load_scene")(e.ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY and f"mesh {a}" in api.last_error()
    assert api.raw("upload_scene")(e.ctx, d.h) == F.HK_E_NOT_READY and f"mesh {a}" in api.last_error()
    assert api.raw("multi_add_meshes")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    assert snap() == before
    assert hip.hipFree(block) == 0
    cam, lights, s = view()
    render_and_compare([gpu, control], cam, s, lights, (1, 2), "after the refusals")
    # n == 0 with no unresolved mesh IS hk_add_meshes
    assert api.raw("add_meshes_device")(control.engine.ctx, plain.h, None, 0, F.TREE_SAH, None) == F.HK_OK
    assert control.engine.last_add() == (0, 0, 0, 0, 0)
    small = of_soup(33, 44)
    host_add(plain, small, True)
    plain.finish()
    assert api.raw("add_meshes_device")(control.engine.ctx, plain.h, None, 0, F.TREE_SAH, None) == F.HK_OK
    assert control.engine.last_add()[:2] == (1, 33) and control.engine.last_add_sources() == (0, 0, 0, RECORD_BYTES(small))
    # an index tensor of a wider type is refused by the wrapper, not narrowed (a value >= 2^31 would wrap)
    with pytest.raises(ValueError):
        gpu.add_meshes(d, sources={a: dict(good[a], indices=good[a]["indices"].to(torch.int64)), b: good[b]})
    assert snap() == before
    # ... and the good table goes through
    gpu.add_meshes(d, sources=good)
    assert d.unresolved_meshes() == 0 and e.last_add_sources()[:3] == (2, 64 + 9, 1)


# ---------------------------------------------------------------------------------------------------------------- 5. producer ordering
@MODES
def test_the_producer_stream_is_ordered_before_and_after_the_call(threaded):
    torch = torch_()
    (d, mat, _), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    s = spec(*S.cloth_grid(9, 7)[0:4:3], seed=51)
    m = declare(d, s)
    assert twin_add(t, s) == m
    d.finish()
    final = source(s)
    half = {k: v * 0.5 for k, v in final.items() if k != "indices"}   # (x 2 on the device is exact)
    busy = torch.randn((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(0)
    with torch.cuda.stream(stream):
        for _ in range(8):                       # the producing kernels are queued behind work that takes a while
            busy = torch.mm(busy, busy) * 1e-3
        made = {k: v * 2.0 for k, v in half.items()}
        made["indices"] = final["indices"] + 0
        gpu.add_meshes(d, sources={m: made}, producer_stream=stream)
        for v in made.values():                  # overwritten in stream order right after the call
            v.fill_(-7 if v.dtype == torch.int32 else float("nan"))
    stream.synchronize()
    t.finish()
    assert_builders_equal(d, t, "sources produced on a side stream")
    instance_all(gpu, twin, d, t, mat, [m])
    nodes_equal(gpu, twin, "a side stream")
    geometry_equal(gpu, twin, t, [m], "a side stream")


# ---------------------------------------------------------------------------------------------------------------- 6. the LDS copy
@MODES
def test_cornell_takes_the_full_layout(threaded):
    dev, tw = hk.load_cornell(), hk.load_cornell()
    d, t = dev.builder, tw.builder
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(dev)
    gpu.engine.read_mesh_nodes()
    specs = [of_soup(2, 61), of_soup(2000, 62)]
    ids = [declare(d, q) for q in specs]
    assert ids == [twin_add(t, q) for q in specs]
    d.finish()
    gpu.add_meshes(d, sources={m: source(q, how) for m, q, how in zip(ids, specs, ("sliced", "packed"))})
    assert gpu.engine.last_add()[:2] == (2, 2002) and gpu.engine.last_add()[4] == 0 and gpu.engine.last_add_sources()[:3] == (2, 2002, 1)
    assert d.unresolved_meshes() == 0
    t.finish()
    assert_builders_equal(d, t, "cornell")
    for b in (d, t):
        for k, m in enumerate(ids):
            b.add_instance(m, 0, S._trs((0.2 * k, 1.0, 0.0), (0.0, 0.0, 0.0), (0.3, 0.3, 0.3)))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    t.finish()
    twin.set_scene(t.finish())
    nodes_equal(gpu, twin, "cornell + 2 + 2000")
    assert gpu.engine.traversal_mode() == twin.engine.traversal_mode()
    render_and_compare([gpu, twin], hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS), None, (1, 2), "cornell + 2 + 2000")


# ---------------------------------------------------------------------------------------------------------------- 7. in flight
@MODES
def test_an_add_that_relocates_with_eight_frames_in_flight(threaded):
    (d, mat, _), (t, _, _), (plain, _, _) = base_builder(), base_builder(), base_builder()
    gpu, twin, without = plugin(threaded), plugin(threaded), plugin(threaded)
    cam, lights, s = view()
    gpu.set_scene(d.scene())
    without.set_scene(plain.scene())
    q = of_soup(900, 71)
    m = declare(d, q)
    assert twin_add(t, q) == m
    d.finish()
    t.finish()
    twin.set_scene(t.scene())   # every mesh from the start, the new one without an instance yet
    src = source(q, "sliced")
    torch_().cuda.synchronize()
    for n in range(1, 9):
        gpu.render(cam, s, lights=lights, frame_number=n)   # (no wait in between)
    gpu.add_meshes(d, sources={m: src})
    assert gpu.engine.last_add()[4] == 1 and gpu.engine.last_add_sources()[:3] == (1, 900, 1)
    frame8 = snapshot(gpu)
    for b in (d, t):
        b.add_instance(m, mat, place(2))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    for n in range(9, 13):
        gpu.render(cam, s, lights=lights, frame_number=n)
    for n in range(1, 9):
        without.render(cam, s, lights=lights, frame_number=n)
        twin.render(cam, s, lights=lights, frame_number=n)
    assert diff_buffers(frame8, snapshot(without)) == {}, "frame 8, read after the add, differs from a run without the add"
    twin.engine.update_instances_on_device(t, F.TREE_SAH)
    for n in range(9, 13):
        twin.render(cam, s, lights=lights, frame_number=n)
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad


# ---------------------------------------------------------------------------------------------------------------- 8. life afterwards
@MODES
def test_life_afterwards_is_that_of_a_host_added_mesh(threaded):
    """The twin context receives the same mesh from host arrays through hk_add_meshes, and both are driven the same way."""
    torch = torch_()
    (d, mat, _), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    p, _, _, i = S.cloth_grid(8, 6)
    q = spec(p, i, seed=81)
    runs = []
    for plug, b, how in ((gpu, d, "device"), (twin, t, "host")):
        plug.set_scene(b.scene())
        plug.engine.read_mesh_nodes()
        if how == "device":
            m = declare(b, q)
            b.finish()
            plug.add_meshes(b, sources={m: source(q, "sliced")})
        else:
            m = host_add(b, q, True)
            b.finish()
            plug.add_meshes(b)
        b.add_instance(m, mat, place(3))
        plug.engine.update_instances_on_device(b, F.TREE_SAH)
        runs.append((plug, b, m))
    assert_builders_equal(d, t, "after the two adds")
    cam, lights, s = view()
    index = d.mesh_index(runs[0][2])
    frame = 1

    def same(what):
        nonlocal frame
        nodes_equal(gpu, twin, what)
        geometry_equal(gpu, twin, d, [runs[0][2]], what)
        render_and_compare([gpu, twin], cam, s, lights, (frame,), what)
        frame += 1

    same("the added mesh")
    bent = p.copy()
    bent[:, 1] = (0.2 * np.sin(5.0 * p[:, 0]) * np.cos(3.0 * p[:, 2])).astype(np.float32)
    for plug, _, _ in runs:
        plug.engine.deform_meshes([("vertices", index, torch.from_numpy(bent).to("cuda:0"), None, dict(recompute_normals=True))])
    same("hk_deform_meshes_device with recomputed normals")
    for plug, _, _ in runs:
        plug.engine.rebuild_mesh_tree(index, F.TREE_SAH)
    same("hk_rebuild_mesh_tree")
    for plug, _, _ in runs:
        plug.engine.set_mesh_motion_vectors(index)
        plug.engine.deform_meshes([("vertices", index, torch.from_numpy((bent * np.float32(1.25)).astype(np.float32)).to("cuda:0"), None, dict(recompute_normals=True))])
    same("hk_set_mesh_motion_vectors and a deformation")
    for plug, b, m in runs:   # the stale state: update_instances_on_device is refused, hk_change_scene_instances is not
        b.add_instance(m, mat, place(7))
        plug.engine.change_instances(b, F.TREE_SAH)
    same("hk_change_scene_instances adding an instance of it")
    for plug, b, m in runs:
        n = len(b.origins)
        b.remove_instance(n - 1)
        b.remove_instance(n - 2)
        plug.engine.change_instances(b, F.TREE_SAH)
        extent = b.remove_mesh(m)
        plug.remove_meshes([extent])
        b.finish()
    nodes_equal(gpu, twin, "hk_remove_meshes of it")
    render_and_compare([gpu, twin], cam, s, lights, (frame,), "hk_remove_meshes of it")
    assert_builders_equal(d, t, "after the removal")
