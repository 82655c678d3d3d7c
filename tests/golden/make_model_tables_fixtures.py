"""Writes the fixtures of tests/test_model_tables_cpu.py:

  tests/golden/model_tables_models.json   flat mh_model_desc form of the small models that test compiles (the three registered ones are
                                          under mecano_amd/models/ already)
  tests/golden/model_tables.json          per model: SHA-256 of every table mh_model_create derives from the description, the scalars,
                                          warning bits and texts verbatim

model_tables.json was written ONCE, from a library whose compile_model was the text of mh_model_create moved unchanged: it pins the
tables to what model creation produced before the restructuring.  A table that differs from it is a finding in compile_model (a reordered
loop or sum), never a reason to run this script again; run it for a NEW model only (it refuses to change an entry that exists).
Data only; mechanisms drawn with numpy and this repository's own generators.
python tests/golden/make_model_tables_fixtures.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

FIELDS_INT = ("parent", "joint_type", "dof_indices", "cfg_indices")
FIELDS_F64 = ("axis", "X_before", "X_com", "inertia_J", "inertia_mass", "inertia_com")
NDOF = {0: 1, 1: 1, 2: 6, 3: 0, 4: 3, 5: 3}
NCFG = {0: 1, 1: 1, 2: 7, 3: 0, 4: 3, 5: 4}


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def pose(rng):
    return np.concatenate([rotation(rng).reshape(-1), rng.uniform(-0.5, 0.5, 3)])


def flat_model(rng, parent, kinds, nq=None, nv=None, dof_indices=None, cfg_indices=None):
    n = len(parent)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    a = rng.normal(size=(n, 3, 3))
    doc = {"n_joints": n, "parent": list(parent), "joint_type": list(kinds), "axis": axis.reshape(-1).tolist(),
           "X_before": np.concatenate([pose(rng) for _ in range(n)]).tolist(), "X_com": np.concatenate([pose(rng) for _ in range(n)]).tolist(),
           "inertia_J": (a @ a.transpose(0, 2, 1) + 0.1 * np.eye(3)).reshape(-1).tolist(), "inertia_mass": rng.uniform(0.1, 2.0, n).tolist(),
           "inertia_com": rng.uniform(-0.3, 0.3, 3 * n).tolist()}
    tv, tq = sum(NDOF[k] for k in kinds), sum(NCFG[k] for k in kinds)
    doc["nv"], doc["nq"] = tv if nv is None else nv, tq if nq is None else nq
    doc["dof_indices"] = list(range(tv)) if dof_indices is None else [int(x) for x in dof_indices]
    doc["cfg_indices"] = list(range(tq)) if cfg_indices is None else [int(x) for x in cfg_indices]
    return doc


def flat_of_desc(desc):
    doc = {"n_joints": int(desc.n_joints), "nq": int(desc.nq), "nv": int(desc.nv)}
    for f in FIELDS_INT:
        doc[f] = [int(x) for x in np.asarray(getattr(desc, f)).reshape(-1)]
    for f in FIELDS_F64:
        doc[f] = [float(x) for x in np.asarray(getattr(desc, f), dtype=np.float64).reshape(-1)]
    return doc


def small_models():
    from test_gpu_edge_cases import _chain_with_axes, _unit
    from mecano_amd import random_tools as rt
    rng = np.random.default_rng(20261018)
    kinds = [2, 0, 1, 3, 4, 5, 0, 1]  # every joint kind, on a tree that branches at the floating root and below the planar joint
    parent = [-1, 0, 1, 0, 3, 4, 4, 2]
    tv, tq = sum(NDOF[k] for k in kinds), sum(NCFG[k] for k in kinds)
    models = {
        "one_revolute": flat_model(rng, [-1], [0]),
        "one_fixed": flat_model(rng, [-1], [3]),
        "chain2": flat_model(rng, [-1, 0], [0, 0]),
        # body 0 has three children: a leaf, a child with a subtree, a leaf (in the caller's order)
        "star": flat_model(rng, [-1, 0, 0, 0, 2], [0, 0, 1, 0, 0]),
        # index maps that are a permutation into wider matrices: three rows of each stay unused
        "every_kind_permuted": flat_model(rng, parent, kinds, nq=tq + 3, nv=tv + 3, dof_indices=rng.permutation(tv + 3)[:tv],
                                          cfg_indices=rng.permutation(tq + 3)[:tq]),
        "forest2": flat_model(rng, [-1, 0, -1, 2, 2], [0, 1, 2, 0, 0]),
    }
    # the two models of tests/test_gpu_edge_cases.py that make mh_model_create warn
    inside = [_unit((1, 3e-8, -4e-8)), _unit((5e-8, 1, 0)), _unit((0, -6e-8, 1)), _unit((1, 0, 9e-8)), _unit((2e-8, 1, 2e-8)), _unit((7e-8, 0, 1)),
              _unit((1, -5e-8, 5e-8))]
    models["near_axis"] = flat_of_desc(_chain_with_axes(np.random.default_rng(8), inside).toModelDesc())
    rng9 = np.random.default_rng(9)
    axes = [rt.nextUnitVector3D(rng9) for _ in range(6)]
    models["tiny_composite"] = flat_of_desc(_chain_with_axes(rng9, axes, tiny_mass_bodies=(4, 5), tiny=4.0e-8).toModelDesc())
    return models


def main():
    import test_model_tables_cpu as t
    from mecano_amd import _lib
    models_path, tables_path = os.path.join(HERE, "model_tables_models.json"), os.path.join(HERE, "model_tables.json")
    stored = json.load(open(models_path)) if os.path.exists(models_path) else {}
    for name, doc in small_models().items():
        stored.setdefault(name, doc)
    with open(models_path, "w") as f:
        json.dump(stored, f)
    pinned = json.load(open(tables_path))["models"] if os.path.exists(tables_path) else {}
    lib = _lib.load()
    for name in t.MODELS:
        if name not in pinned:
            pinned[name] = t.digest(t.tables_of(lib, t.model_desc(name)))
            print("pinned", name, pinned[name]["scalars"])
    with open(tables_path, "w") as f:
        json.dump({"comment": "Tables of mh_model_create (ModelTables, mecano_amd/csrc/mh_model_tables.h) per model, from the statements of model creation "
                              "as they stood before they were split into steps; tests/golden/make_model_tables_fixtures.py.", "models": pinned}, f, indent=1)
    print(models_path, os.path.getsize(models_path), "bytes;", tables_path, os.path.getsize(tables_path), "bytes")


if __name__ == "__main__":
    main()
