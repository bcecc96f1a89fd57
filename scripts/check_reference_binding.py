#!/usr/bin/env python3
"""BUILD-CONTAINER check (needs /root/reference; never runs on the GPU box): the reference's OWN caller code binds to the drop-ins.

`gsn_amd/dropin` is put in front of /root/reference on sys.path -- the integration route of INTEGRATION.md 1 -- and the reference's
unchanged `utils.py` is imported from /root/reference.  Its import statements (utils.py:2-5) then resolve utils_graph_processing /
utils_ids / utils_data_gen / utils_graph_learning to this package, and its host-only logic runs over them:

  * `process_arguments` (utils.py:35-92) picks `count_fn`, `automorphism_fn`, `extract_id_fn` for id_scope local / global and
    edge_automorphism induced / line_graph: asserted to BE this package's functions, with the `__name__` strings utils_data_gen.py:103
    compares against;
  * `get_custom_edge_list` (utils.py:16-33) builds the pattern families (cycle_graph, complete_graph, path_graph, star_graph,
    all_simple_graphs from the reference's .g6 files, ...);
  * the `subgraph_dicts` construction of utils_data_gen.py:35-42 (the same four-tuple unpacking, `len(orbit_partition)`) is run over the
    selected `automorphism_fn` for every pattern, and the tables are compared with tests/golden/orbits.npz (produced by the reference's
    own functions over networkx VF2).

No device is touched (orbits are host code: csrc/patterns.cpp).  Exit code 0 and "binding ok" on success.
    python scripts/check_reference_binding.py

`--record` also writes what the run saw to tests/golden/reference_binding.json: the names utils.py takes from the drop-in modules, and
per case the functions process_arguments selected (by name) and the pattern edge lists it built.  `--recorded [FILE]` needs no reference:
it resolves those names over gsn_amd/dropin and runs the same selection and orbit-table checks on the recorded patterns
(tests/test_dropin_cpu.py).
    python scripts/check_reference_binding.py --record
    python scripts/check_reference_binding.py --recorded"""
import importlib
import json
import os
import sys
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
DROPIN = os.path.join(REPO, "gsn_amd", "dropin")
RECORD = os.path.join(REPO, "tests", "golden", "reference_binding.json")
FAMILIES = [("cycle_graph", [8], "cycle_graph", 0), ("complete_graph", [6], "complete_graph", 0), ("path_graph", [6], "path_graph", 0),
            ("star_graph", [5], "star_graph", 0), ("diamond_graph", [4], "diamond_graph", 0),
            ("all_simple_graphs", [5], None, 0), ("all_simple_graphs_chosen_k", [5], "all_simple_graphs_5", 0),
            ("cycle_graph_chosen_k", [4, 6], "cycle_graph", None)]
DROPIN_MODULES = ("utils_graph_processing", "utils_ids", "utils_data_gen", "utils_graph_learning", "utils_encoding", "models_misc")


def _name(fn):
    return fn.__module__ + "." + fn.__name__


def _resolve(qual):
    mod, name = qual.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


def _want():
    import gsn_amd.counting as gc
    import gsn_amd.patterns as gp
    return {("local", "induced"): (gc.subgraph_isomorphism_edge_counts, gp.induced_edge_automorphism_orbits),
            ("global", "induced"): (gc.subgraph_isomorphism_vertex_counts, gp.automorphism_orbits),
            ("local", "line_graph"): (gc.subgraph_isomorphism_edge_counts, gp.edge_automorphism_orbits),
            ("global", "line_graph"): (gc.subgraph_isomorphism_vertex_counts, gp.automorphism_orbits)}


def check_selection(scope, autom, extract_id_fn, count_fn, automorphism_fn):
    """What process_arguments (utils.py:35-92) selected is this package's function, with the names utils_data_gen.py:103 compares."""
    import gsn_amd.counting as gc
    count_want, aut_want = _want()[(scope, autom)]
    assert extract_id_fn is gc.subgraph_counts2ids
    assert count_fn is count_want, (scope, autom, count_fn)
    assert automorphism_fn is aut_want, (scope, autom, automorphism_fn)
    assert count_fn.__name__ == ("subgraph_isomorphism_edge_counts" if scope == "local" else "subgraph_isomorphism_vertex_counts")


def check_tables(scope, autom, id_type, k, fixture, edge_lists, automorphism_fn, z):
    """utils_data_gen.py:35-42, statement for statement over the selected function, against the reference-generated tables of orbits.npz;
    returns the number of pattern tables compared."""
    if autom == "line_graph" and scope == "local":
        return 0                                      # (deprecated path: covered by test_line_graph_edge_orbits_match_reference)
    subgraph_dicts, orbit_partition_sizes = [], []
    for edge_list in edge_lists:
        subgraph, orbit_partition, orbit_membership, aut_count = automorphism_fn(edge_list=edge_list, directed=False, directed_orbits=False)
        subgraph_dicts.append({'subgraph': subgraph, 'orbit_partition': orbit_partition, 'orbit_membership': orbit_membership, 'aut_count': aut_count})
        orbit_partition_sizes.append(len(orbit_partition))
    if id_type == "all_simple_graphs":
        keys = ["all_simple_graphs_%d/%d" % (kk, i) for kk in (3, 4, 5) for i in range(sum(1 for f in z.files if f.startswith("all_simple_graphs_%d/" % kk) and f.endswith("/edges")))]
    elif id_type == "cycle_graph_chosen_k":
        keys = ["cycle_graph/%d" % (kk - 3) for kk in k]
    else:
        keys = ["%s/%d" % (fixture, i) for i in range(len(edge_lists))]
    assert len(keys) == len(edge_lists), (id_type, len(keys), len(edge_lists))
    for key, el, d in zip(keys, edge_lists, subgraph_dicts):
        assert [list(e) for e in el] == z[key + "/edges"].tolist(), key
        assert int(d['aut_count']) == int(z[key + "/aut_count"]), key
        memb = d['orbit_membership']
        if scope == "global":
            assert [int(memb[v]) for v in sorted(memb)] == z[key + "/v_membership"].tolist(), key
            assert len(d['orbit_partition']) == int(z[key + "/n_vorbits"]), key
        else:
            arcs = z[key + "/e_list"].tolist()
            # (the reference keys the edge membership by the index of the arc in its sorted arc list, utils_graph_processing.py:84-98)
            assert [int(memb[i]) for i in range(len(arcs))] == z[key + "/e_membership"].tolist(), key
            assert sorted(tuple(a) for p_ in d['orbit_partition'].values() for a in p_) == sorted(tuple(a) for a in arcs), key
            assert len(d['orbit_partition']) == int(z[key + "/n_eorbits"]), key
    return len(keys)


def check_star8(scope, el, automorphism_fn, zs):
    """--id_type star_graph --k 8 (utils.py:59-62): its largest pattern has NINE vertices (GSN_KMAX 8 -> 9 in r06); tables of counts_stars.npz"""
    assert [list(e) for e in el] == zs["star8/edges"].tolist()
    subgraph, orbit_partition, orbit_membership, aut_count = automorphism_fn(edge_list=el, directed=False, directed_orbits=False)
    assert int(aut_count) == int(zs["star8/aut_count"]) == 40320
    key = "star8/v_membership" if scope == "global" else "star8/e_membership"
    assert [int(orbit_membership[i]) for i in range(len(orbit_membership))] == zs[key].tolist()


def _goldens():
    return (np.load(os.path.join(REPO, "tests", "golden", "orbits.npz"), allow_pickle=False),
            np.load(os.path.join(REPO, "tests", "golden", "counts_stars.npz"), allow_pickle=False))


def main_recorded(path):
    """No reference needed: what the reference's utils.py imported and selected, as recorded by --record (names and pattern edge lists),
    resolved over gsn_amd/dropin and checked the same way as the live run."""
    sys.path[:0] = [DROPIN, REPO]
    with open(path) as f:
        rec = json.load(f)
    mods = {m: importlib.import_module(m) for m in DROPIN_MODULES}
    for m in mods.values():
        assert m.__file__.startswith(DROPIN), m.__file__
    # the names utils.py takes from the drop-in modules (utils.py:2-5): each one is there, and is the gsn_amd object it was in the reference run
    for name, (src, defined_in) in sorted(rec["imports"].items()):
        obj = getattr(mods[src], name)
        target = _resolve(defined_in + "." + name)
        assert target is obj or getattr(obj, "__wrapped__", None) is target, (name, src, defined_in)     # (generate_dataset: a wrapper)
    import gsn_amd.counting as gc
    import gsn_amd.dataset as gd
    assert mods["utils_ids"].subgraph_counts2ids is gc.subgraph_counts2ids
    assert mods["utils_data_gen"].generate_dataset.__wrapped__ is gd.generate_dataset
    z, zs = _goldens()
    n_patterns = 0
    seen = set()
    for c in rec["cases"]:
        fns = [_resolve(c[k]) for k in ("extract_id_fn", "count_fn", "automorphism_fn")]
        check_selection(c["scope"], c["autom"], *fns)
        assert getattr(mods["utils_graph_processing"], fns[2].__name__) is fns[2]     # (reached through the drop-in, as utils.py does)
        edge_lists = [[tuple(e) for e in el] for el in c["edge_lists"]]
        n_patterns += check_tables(c["scope"], c["autom"], c["id_type"], c["k"], c["fixture"], edge_lists, fns[2], z)
        seen.add((c["scope"], c["autom"], c["id_type"]))
    assert seen == {(s, a, f[0]) for (s, a) in _want() for f in FAMILIES}, "the record does not cover every case"
    for c in rec["star8"]:
        check_star8(c["scope"], [tuple(e) for e in c["edge_list"]], _resolve(c["automorphism_fn"]), zs)
        n_patterns += 1
    assert sorted(c["scope"] for c in rec["star8"]) == ["global", "local"]
    print("binding ok: recorded selections of the reference's utils.process_arguments over gsn_amd/dropin, %d pattern tables equal to orbits.npz"
          % n_patterns)


def main():
    if "--recorded" in sys.argv:
        return main_recorded(sys.argv[sys.argv.index("--recorded") + 1] if len(sys.argv) > sys.argv.index("--recorded") + 1 else RECORD)
    if not os.path.isdir(REF):
        raise SystemExit("needs the reference checkout at REF; --recorded checks the committed record instead")
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_golden                                   # (its stubs of torch_geometric / ogb / graph_tool: what utils.py imports but this check never calls)
    make_golden.install_stubs()
    sys.modules.pop("graph_tool", None)                  # the drop-ins must not need graph-tool at all
    sys.path[:0] = [DROPIN, REPO]
    sys.path.append(REF)                                 # BEHIND the drop-ins: what they do not shadow (utils.py, utils_misc.py, ...) comes from the reference
    import utils                                         # the reference's utils.py, unchanged
    assert utils.__file__ == os.path.join(REF, "utils.py"), utils.__file__
    import gsn_amd.counting as gc
    import gsn_amd.dataset as gd
    import utils_graph_processing as ugp
    assert ugp.__file__.startswith(DROPIN), ugp.__file__
    assert utils.subgraph_counts2ids is gc.subgraph_counts2ids
    assert utils.generate_dataset.__wrapped__ is gd.generate_dataset
    record = {"imports": {}, "cases": [], "star8": []}
    mods = {m: importlib.import_module(m) for m in DROPIN_MODULES}
    for name, obj in vars(utils).items():
        src = [m for m, mod in mods.items() if getattr(mod, name, None) is obj and not name.startswith("__")]
        if src and callable(obj):
            record["imports"][name] = [src[0], obj.__module__]

    base = dict(inject_degrees=False, degree_as_tag=False, retain_features=True, num_layers=4, d_msg=None, d_out=64, d_h=None,
                num_mlp_layers=2, d_out_edge_encoder=None, d_out_node_encoder=None, d_out_id_embedding=None, d_out_degree_embedding=None,
                root_folder=os.path.join(REF, "datasets"), custom_edge_list=None, vn=False, train_eps=False, final_projection=[True], bn=True,
                dropout_features=0.0, loss_fn="L1Loss", prediction_fn="L1Loss", regression=True)
    z, zs = _goldens()
    n_patterns = 0
    for (scope, autom) in _want():
        for id_type, k, fixture, _ in FAMILIES:
            args = dict(base, id_scope=scope, edge_automorphism=autom, id_type=id_type, k=list(k))
            res = utils.process_arguments(args)
            args_out, extract_id_fn, count_fn, automorphism_fn = res[0], res[1], res[2], res[3]
            check_selection(scope, autom, extract_id_fn, count_fn, automorphism_fn)
            edge_lists = args_out["custom_edge_list"]
            record["cases"].append({"scope": scope, "autom": autom, "id_type": id_type, "k": list(k), "fixture": fixture,
                                    "extract_id_fn": _name(extract_id_fn), "count_fn": _name(count_fn), "automorphism_fn": _name(automorphism_fn),
                                    "edge_lists": [[[int(a), int(b)] for a, b in el] for el in edge_lists]})
            n_patterns += check_tables(scope, autom, id_type, k, fixture, edge_lists, automorphism_fn, z)
    for scope in ("global", "local"):
        args = dict(base, id_scope=scope, edge_automorphism="induced", id_type="star_graph", k=[8])
        res = utils.process_arguments(args)
        el = res[0]["custom_edge_list"][-1]
        check_star8(scope, el, res[3], zs)
        record["star8"].append({"scope": scope, "automorphism_fn": _name(res[3]), "edge_list": [[int(a), int(b)] for a, b in el]})
        n_patterns += 1
    if "--record" in sys.argv:
        with open(RECORD, "w") as f:
            json.dump(record, f, separators=(",", ":"))
            f.write("\n")
    print("binding ok: reference utils.process_arguments / get_custom_edge_list over gsn_amd/dropin, %d pattern tables equal to orbits.npz" % n_patterns)


if __name__ == "__main__":
    main()
