"""The gate of the table arm of the key path (gsn_amd.step.tables_path_ok) and the library's table shape, without a GPU."""
import pytest


@pytest.mark.parametrize("n_classes,clamp,ok", [([28], True, True), ([28], False, True), ([30], False, True), ([31], True, True), ([31], False, False),
                                                ([32], True, False), ([1, 5, 6], True, True), ([4, 8], True, False), ([5, 5], False, False),
                                                ([4, 5], False, True), ([31, 1], True, True), ([16, 2], True, False), ([7, 7, 6], True, False)])
def test_gate_is_the_dictionary_row_count(n_classes, clamp, ok):
    """31 rows against 32, clamped and with the "none" digit; beyond 256 rows neither key arm runs"""
    import numpy as np
    from gsn_amd.step import TABLE_ROWS, keys_path_ok, node_key_radices, tables_path_ok
    rows = int(np.prod(node_key_radices(n_classes, clamp)))
    assert tables_path_ok(n_classes, clamp) == ok == (rows <= TABLE_ROWS)
    assert not tables_path_ok(n_classes, clamp) or keys_path_ok(n_classes, clamp)


def test_gate_does_not_depend_on_the_weights():
    """The tables hold the edge stage's x_i products, a function of the target's dictionary row for ANY weights.  A zero degree column of the
    folded node-stage-0 weight, [W3x | W3a W2 | W3a b2 | 0 0 0], would only matter to a table of node stage 0's [x | deg] chunks, which is not
    built: that column is W3a b2, non-zero for the default initialisation of the layer (and so at the benchmark)."""
    import inspect
    import torch
    from gsn_amd import layers, step
    assert list(inspect.signature(step.tables_path_ok).parameters) == ["n_classes", "clamp"]
    layer = layers.GSN_edge_sparse(d_in=28, d_ef=4, d_id=12, d_degree=1, degree_as_tag=False, retain_features=True, id_scope="local", d_msg=128,
                                   d_up=128, d_h=[128], seed=0, activation_name="relu", bn=True, msg_kind="general", flow="source_to_target").eval()
    deg_col = layer.update_fn.fc[0].weight[:, 28:].detach() @ layer.msg_fn.fc[-1].bias.detach()
    assert float(deg_col.abs().max()) > 0


def test_library_tables_match_the_gate_constant():
    from gsn_amd import _abi
    from gsn_amd.step import TABLE_ROWS
    L = _abi.lib()
    assert int(L.gsn_layer_key_tables_max_rows()) == TABLE_ROWS and int(L.gsn_layer_key_tables_words()) == 4 * TABLE_ROWS * 32


def test_switch_is_in_the_table():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gsn_amd", "csrc", "switches.h")).read()
    assert "X(RP_TABLES, LIVE," in src
