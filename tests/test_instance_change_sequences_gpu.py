"""Seeded sequences that interleave what makes the host's mirrors stale - deformations, poses from device tensors - with mesh additions and
removals and with instance-set edits through hk_change_scene_instances, on the two-slot base scene of tests/scene_edit_model.py.  The
generator is a small one of its own: the model's legality table describes hk_update_scene_instances, which is refused in these states; every
op here is one the new call's contract accepts.  The end state - after the closing step of tests/test_scene_edit_sequences_gpu.py: every
instance at rest, both trees rebuilt - is compared with the twin of tests/test_instance_change_gpu.py: emitters, trees, poses, two frames."""
import numpy as np
import pytest

import scene_edit_model as M
from test_instance_change_gpu import BASE, GLOW, Side, against_twin

pytestmark = pytest.mark.gpu

SEEDS = list(range(8))
MAX_OPS = 12
DEFORMS = {"cloth": "vertices", "sphere": "vertices", "s7": "vertices", "cylinder": "skin", "s1": "vertices", "s3": "vertices"}
ARRIVALS = ("s1", "s2", "s3", "s300")
KEPT = ("s1100",)                 # keeps the scene beyond the LDS copy
NEVER_INSTANCED = ("s40",)        # no instance at load: its tree has no leaf boxes until a host layout gives it one


def generate(seed):
    """ops as (kind, arguments), decided against a shadow of the instance list so that every op is legal when it runs"""
    rng = np.random.default_rng(9000 + seed)
    d = M.base_description(BASE)
    names = [n for n, _ in d["meshes"]]
    inst = [n for n, _, _ in d["instances"]]
    ops, serial = [], 0
    for _ in range(int(rng.integers(8, MAX_OPS + 1))):
        kind = rng.choice(["deform", "poses", "instances", "instances", "add_mesh", "remove_mesh", "frame"])
        serial += 1
        if kind == "deform":
            choices = [n for n in DEFORMS if n in inst]
            if choices:
                ops.append(("deform", str(rng.choice(choices)), serial))
        elif kind == "poses":
            if rng.random() < 0.5:
                ops.append(("poses", None, [100 * serial + k for k in range(len(inst))]))
            else:
                ids = sorted(rng.choice(len(inst), size=int(rng.integers(1, len(inst) + 1)), replace=False).tolist(), reverse=True)
                ops.append(("poses", ids, [100 * serial + k for k in range(len(ids))]))
        elif kind == "instances":
            edits = []
            for k in range(int(rng.integers(1, 5))):
                what = rng.choice(["add", "remove", "material"]) if len(inst) > 1 else "add"
                if what == "add":
                    name = str(rng.choice([n for n in names if n not in NEVER_INSTANCED]))
                    edits.append(("add", name, int(rng.integers(0, 4)), 100 * serial + 50 + k))
                    inst.append(name)
                elif what == "remove":
                    i = int(rng.integers(0, len(inst)))
                    edits.append(("remove", i))
                    del inst[i]
                else:
                    edits.append(("material", int(rng.integers(0, len(inst))), int(rng.integers(0, 4))))
            ops.append(("instances", edits))
        elif kind == "add_mesh":
            choices = [n for n in ARRIVALS if n not in names]
            if choices:
                name = str(rng.choice(choices))
                ops.append(("add_mesh", name, int(rng.integers(0, 4)), 100 * serial + 60))
                names.append(name)
                inst.append(name)
        elif kind == "remove_mesh":
            choices = [n for n in names if n not in KEPT and any(i != n for i in inst)]
            if choices:
                name = str(rng.choice(choices))
                ops.append(("remove_mesh", name))
                names.remove(name)
                inst = [i for i in inst if i != name]
        else:
            ops.append(("frame",))
    return ops


def run(side, op):
    """-> whether the op went through hk_change_scene_instances"""
    kind = op[0]
    if kind == "deform":
        name = op[1]
        if DEFORMS[name] == "skin" and name in side.deformed:
            side.e.deform_meshes([("skin", side.index(name), M.joints(op[2]))])
        else:
            side.deform(DEFORMS[name], name, op[2])
    elif kind == "poses":
        side.device_poses(op[2], op[1])
    elif kind == "instances":
        for e in op[1]:
            if e[0] == "add":
                side.add(e[1], e[2], e[3])
            elif e[0] == "remove":
                side.remove(e[1])
            else:
                side.rematerial(e[1], e[2])
        side.change()
        return True
    elif kind == "add_mesh":
        side.add_mesh(op[1])
        side.add(op[1], op[2], op[3])
        side.change()
        return True
    elif kind == "remove_mesh":
        gone = [k for k, (n, _) in enumerate(side.inst) if n == op[1]]
        if gone:
            for k in reversed(gone):
                side.remove(k)
            side.change()
        side.remove_mesh(op[1])
        return bool(gone)
    else:
        side.render()
    return False


@pytest.mark.parametrize("seed", SEEDS)
def test_a_sequence_with_instance_changes_leaves_what_the_twin_loaded(seed):
    ops = generate(seed)
    assert len(ops) <= MAX_OPS
    side = Side(seed % 2 == 1)
    stale = False
    for op in ops:
        if run(side, op):
            took_host_path = bool(side.e.last_instance_change()[3] & 2)
            assert took_host_path == (not stale), (seed, op, side.e.last_instance_change())
        stale = stale or op[0] in ("deform", "poses")
    side.settle()
    emitters = sum(1 for _, m in side.inst if m == GLOW)
    against_twin(side, f"seed {seed}: {ops}", emitters=emitters)
