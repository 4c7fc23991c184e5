"""The scene-edit model (tests/scene_edit_model.py) without a GPU: the builder held against itself over seeded sequences, the coverage of
the seed list the GPU tests run (computed here, not assumed), and the model's determinism across processes."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import scene_edit_model as M
from bevy_hikari_amd import _ffi as F
from conftest import ROOT

BUFFERS = ("vertices", "primitives", "asset_nodes", "materials", "instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table")

#: the seeds of tests/test_scene_edit_sequences_gpu.py, chosen (greedily, from 0 .. 399) so that test_the_seed_list_covers_the_vocabulary holds
SEEDS = dict(two_slot=(0, 2, 11, 13, 14, 131, 140, 167, 302, 338), one_slot=(0, 1, 28, 51, 169, 185, 245, 293, 307))
#: three of the two-slot seeds run through a two-band MultiEngine as well, with the vocabulary the multi wrapper has
BAND_SEEDS = (2, 11, 13)


def length_of(seed):
    """12 to 20 ops"""
    return 12 + (7 * seed) % 9


def sequence(seed, base, kinds=M.KINDS):
    return M.generate(seed, base, length_of(seed), kinds)


# ---------------------------------------------------------------------------------------------------------------- 1. the builder against itself
def rebase(extents, index):
    arr = (F.HkMeshExtent * max(1, len(extents)))(*extents)
    out = F.HkMeshIndex()
    F.api().call("rebase_mesh_index", arr, len(extents), C.byref(index), C.byref(out))
    return out


def apply_to_builder(b, state, op):
    """the builder-level part of an accepted op on builder `b` (in `state`, the model's state in front of the op), with a finish behind it"""
    base, k, a = state.base, op.kind, op.args
    if k == "add_meshes":
        for name, how in a["meshes"]:
            M.add_pool_mesh(b, base, name, how)
        b.finish()
        if any(how == "deferred" for _, how in a["meshes"]):
            assert b.pending_mesh_trees() == sum(how == "deferred" for _, how in a["meshes"])
            b.build_pending_mesh_trees()
        names = state.names() + [n for n, _ in a["meshes"]]
        for name, mat, p in a["instances"]:
            b.add_instance(names.index(name), mat, M.pose(base, p))
    elif k == "remove_meshes":
        for i in sorted(a["drop_instances"], reverse=True):
            b.remove_instance(i)
        b.finish()
        survivors = [n for n in state.names() if n not in a["meshes"]]
        old = {n: b.mesh_index(state.mesh_id(n)) for n in survivors}
        extents = [b.remove_mesh(state.mesh_id(n)) for n in sorted(a["meshes"], key=state.mesh_id, reverse=True)]
        b.finish()
        for new_id, n in enumerate(survivors):   # the new record of every survivor: its old one rebased over the extents removed
            assert bytes(b.mesh_index(new_id)) == bytes(rebase(extents, old[n])), (op, n)
    elif k == "add_instance":
        b.add_instance(state.mesh_id(a["mesh"]), a["material"], M.pose(base, op.seed))
    elif k == "remove_instance":
        b.remove_instance(a["instance"])
    elif k == "set_instance_material":
        b.set_instance_material(a["instance"], a["material"])
    elif k in ("refit_instances", "set_instance_transforms"):
        for i, p in a["poses"]:
            b.set_instance_transform(i, M.pose(base, p))
    elif k == "set_material":
        b.set_material(a["material"], M.material(base, a["material"], a["version"]))
    elif k == "update_mesh_vertices":
        M.replay_history_on_host(b, base, state.mesh_id(a["mesh"]), [("vertices", a["mesh"], op.seed, a["normals"])])
    elif k in ("deform_meshes", "deform_meshes_device"):
        for it in a["items"]:
            M.replay_history_on_host(b, base, state.mesh_id(it[1]), [tuple(it)])
    elif k == "rebuild_mesh_tree":
        b.rebuild_mesh_tree(state.mesh_id(a["mesh"]))
    b.finish()


def run_on_builder(ops, base):
    b, state = M.base_builder(base), M.State(base)
    for op in ops:
        if not op.refuse:
            apply_to_builder(b, state, op)
        state.apply(op)
    return b


@pytest.mark.parametrize("base", M.BASES)
def test_the_builder_edited_step_by_step_equals_the_builder_given_the_end_state(base):
    """200 seeds per base scene (400 sequences): every exported array byte for byte, and inside apply_to_builder the record of every survivor
    of every removal against hk_rebase_mesh_index."""
    removals = 0
    for seed in range(1000, 1200):
        ops = sequence(seed, base)
        removals += sum(op.kind == "remove_meshes" and not op.refuse for op in ops)
        got = run_on_builder(ops, base).scene()
        want = M.end_builder(M.end_state(ops, base), True).scene()
        for n in BUFFERS:
            assert bytes(getattr(got, n)) == bytes(getattr(want, n)), f"seed {seed}: {n} differ from the end-state builder's\n" + "\n".join(map(repr, ops))
    assert removals >= 50, removals   # (not vacuous: on one slot removals are legal only while the mirrors are fresh)


# ---------------------------------------------------------------------------------------------------------------- 2. coverage
#: ordered family pairs (A, then later B) the legality table leaves no way to on the SAME mesh or, for scene-wide ops, in one sequence
IMPOSSIBLE_PAIRS = dict(two_slot={}, one_slot={
    ("instance_set", "mesh_set"): "update_instances_on_device ends in hk_rebuild_scene_trees: the mirrors are stale, the full layout is refused",
    ("poses", "mesh_set"): "a refit or a device pose call leaves the mirrors stale",
    ("geometry", "mesh_set"): "a deformation leaves them stale; a mesh with a skin or a morph set leaves only after its instance, whose removal does",
    ("trees", "mesh_set"): "both rebuilds leave them stale"})


def coverage(seeds, base):
    """(per-kind counts of accepted ops, per-pair counts, per-row counts of refusals, sequences with a removal after an add after a removal,
    sequences with a deformation between an add_meshes and the next frame, sequences with an add_meshes between a deformation and the next frame)"""
    kinds = {k: 0 for k in M.KINDS}
    pairs = {(a, b): 0 for a in M.FAMILIES for b in M.FAMILIES}
    rows = {r: 0 for r in M.REFUSAL_ROWS[base]}
    rar = add_deform_frame = deform_add_frame = rekeyed = 0
    for seed in seeds:
        ops = sequence(seed, base)
        seen = set()
        rekeyed += uses_a_set_whose_record_moved(ops, base)
        for j, op in enumerate(ops):
            if op.refuse:
                rows[op.refuse] += 1
                continue
            kinds[op.kind] += 1
            mj = set(op.meshes())
            for i in range(j):
                if ops[i].refuse:
                    continue
                mi = set(ops[i].meshes())
                if not mi or not mj or mi & mj:
                    seen.add((ops[i].family, op.family))
        for p in seen:
            pairs[p] += 1
        ok = [op for op in ops if not op.refuse]
        mesh_ops = "".join("r" if op.kind == "remove_meshes" else "a" for op in ok if op.family == "mesh_set")
        stage = 0
        for c in mesh_ops:
            if (stage in (0, 2) and c == "r") or (stage == 1 and c == "a"):
                stage += 1
        rar += stage >= 3
        for first, second in ((("add_meshes",), M.DEFORMING), (M.DEFORMING, ("add_meshes",))):
            found = False
            for i, op in enumerate(ok):
                if op.kind not in first:
                    continue
                for j in range(i + 1, len(ok)):
                    if ok[j].family == "observers":
                        break
                    if ok[j].kind in second and any(o.kind == "frame" for o in ok[j + 1:]):
                        found = True
            if first == ("add_meshes",):
                add_deform_frame += found
            else:
                deform_add_frame += found
    return kinds, pairs, rows, rar, add_deform_frame, deform_add_frame, rekeyed


def uses_a_set_whose_record_moved(ops, base):
    """a skin, morph or morph + skin item on a mesh whose skin or morph set was given before a removal in front of the mesh moved its record"""
    state, moved = M.State(base), set()
    for op in ops:
        if not op.refuse:
            if op.kind == "remove_meshes":
                first = min(state.mesh_id(n) for n in op.args["meshes"])
                moved |= {n for n in state.skins + state.morphs if state.mesh_id(n) > first}
            if op.kind in ("deform_meshes", "deform_meshes_device") and any(it[0] != "vertices" and it[1] in moved for it in op.args["items"]):
                return True
        state.apply(op)
        moved &= set(state.names())
    return False


@pytest.mark.parametrize("base", M.BASES)
def test_the_seed_list_covers_the_vocabulary(base):
    kinds, pairs, rows, rar, adf, daf, rekeyed = coverage(SEEDS[base], base)
    print(f"{base}: {len(SEEDS[base])} seeds, lengths {sorted({length_of(s) for s in SEEDS[base]})}")
    print("  accepted ops per kind:", kinds)
    print("  sequences per ordered family pair:", {f"{a}>{b}": n for (a, b), n in pairs.items()})
    print("  refusals per row:", rows)
    print(f"  remove-add-remove: {rar}; add, deformation, frame: {adf}; deformation, add, frame: {daf}; a skin or morph set used after its record moved: {rekeyed}")
    assert all(12 <= length_of(s) <= 20 for s in SEEDS[base]) and len(SEEDS[base]) <= 16
    assert min(kinds.values()) >= 3, {k: n for k, n in kinds.items() if n < 3}
    missing = [p for p, n in pairs.items() if n == 0 and p not in IMPOSSIBLE_PAIRS[base]]
    assert not missing, missing
    assert not [p for p in IMPOSSIBLE_PAIRS[base] if pairs[p]], "a pair the table is said to exclude occurs"
    assert min(rows.values()) >= 1, rows
    assert rar >= 1 and adf >= 1
    if base == "two_slot":   # (on one slot the add behind a deformation is a refusal row, and so is the removal behind a skin's first use)
        assert daf >= 1 and rekeyed >= 2
    for seed in BAND_SEEDS:
        assert seed in SEEDS["two_slot"]


def test_the_impossible_pairs_stay_impossible_over_many_seeds():
    """what IMPOSSIBLE_PAIRS lists never occurs in 400 seeds per base scene: the list is the table's, not the seed list's"""
    for base in M.BASES:
        pairs = coverage(range(400), base)[1]
        assert not [p for p in IMPOSSIBLE_PAIRS[base] if pairs[p]]


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
def digests(seeds):
    out = []
    for base in M.BASES:
        for seed in seeds:
            ops = sequence(seed, base)
            out.append(f"{base} {seed} {[op.key() for op in ops]!r} {M.state_digest(M.end_state(ops, base))}")
    return out


def test_the_same_seed_gives_the_same_ops_and_end_state_in_two_processes():
    seeds = [0, 1, 2, 3, 4, 5]
    code = ("import sys; sys.path[:0] = [%r, %r]; import conftest, test_scene_edit_sequences as T; print('\\n'.join(T.digests(%r)))" % (ROOT, os.path.join(ROOT, "tests"), seeds))
    runs = []
    for hashseed in ("1", "2"):
        env = dict(os.environ, PYTHONHASHSEED=hashseed)
        runs.append(subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True, cwd=ROOT).stdout.strip().split("\n"))
    assert runs[0] == runs[1] == digests(seeds)


def test_the_generator_raises_when_it_finds_no_legal_op():
    with pytest.raises(RuntimeError):
        M.generate(0, "two_slot", 4, kinds=())   # (an empty vocabulary: an error, not a shorter sequence)


# ---------------------------------------------------------------------------------------------------------------- 4. regressions
def test_set_mesh_vertices_behind_a_removed_mesh_takes_the_meshs_own_vertex_count():
    """Found by the builder test above: SceneBuilder.remove_mesh left the wrapper's per-id vertex counts unshifted, so set_mesh_vertices on a mesh
    behind the removed one checked its arrays against the count of the mesh that used to have the id."""
    base = "two_slot"
    b, state = M.base_builder(base), M.State(base)
    assert M.n_vertices(base, "s7") != M.n_vertices(base, "cloth")
    b.remove_instance(state.instances_of("s7")[0])
    b.remove_mesh(state.mesh_id("s7"))
    b.finish()
    positions, normals = M.vertex_data(base, "cloth", 3, True)
    b.set_mesh_vertices(state.mesh_id("cloth") - 1, positions, normals)
    b.finish()
