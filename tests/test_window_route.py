"""The device-free part of the window-route rule (models._window_recipe_ok): which resident-series batches `fused_training_step_windows` (training) and
`forward_windows` (evaluation) take, and which go to the assembled route.  One row per condition, each a single change to an accepted input, stating what each
of the two routes does with it; the conditions on the engine, the parameters and the grad mode are pinned by the GPU tests of the window routes."""
import dataclasses
import types

import pytest

from morphsym_hgnn_amd import synth
from morphsym_hgnn_amd.models import _window_recipe_ok
from morphsym_hgnn_amd.windows import quadsdk_a1_c2_recipe, solo_com_recipe
from tests import helpers

JP, FP = list(range(12)), list(range(4))
A1 = helpers.make_spec("c2", "a1-c2", "a1-c2", 128, 2)                   # widths 900 / 450 / 1: a history of 150
SOLO = helpers.make_spec("k4_com", "solo-k4-com", "solo-k4", 128, 2)     # widths 6 / 2: a history of 1


def a1_spec(history):
    return dataclasses.replace(A1, widths=synth.feature_widths("c2", True, history), num_timesteps=history)


def a1(history=150, **kw):
    return quadsdk_a1_c2_recipe(JP, FP, history, 3, **kw)


def desc_of(recipe, fast_layout=1, one_run_per_row=False):
    """The fields of the store's descriptor the rule reads, with the recipe's own run and row counts (one_run_per_row: as if every node row were a single run)."""
    runs, rows, _, _ = recipe.tables()
    return types.SimpleNamespace(fast_layout=fast_layout, n_runs=len(rows) if one_run_per_row else len(runs), n_rows=len(rows))


def solo(history=1, normalize=False):
    return dataclasses.replace(solo_com_recipe("k4_com", JP, history), normalize=normalize)


def solo_spec(recipe):
    """What the rule reads of a spec (node types, node counts, widths) for a Solo model whose widths are the recipe's: ModelSpec itself refuses a Solo model of more
    than one time step, so a recipe with a longer history can only be isolated from the width check on a stand-in."""
    return types.SimpleNamespace(node_types=SOLO.node_types, num_nodes=SOLO.num_nodes, widths={t: recipe.width(t) for t in recipe.node_types})


# (id, spec, recipe, descriptor overrides, store dtype, training takes the route, evaluation takes the route)
ROWS = [
    ("accepted_bf16", A1, a1(), {}, "bf16", True, True),
    ("accepted_x3", A1, a1(), {}, "x3", True, True),
    ("accepted_f32_store", A1, a1(), {}, "f32", True, True),
    ("no_spec_yet", None, a1(), {}, "bf16", False, False),
    ("store_dtype_unknown", A1, a1(), {}, "f16", False, False),
    ("not_fast_layout", A1, a1(), {"fast_layout": 0}, "bf16", False, False),
    ("standardised", A1, a1(normalize=True), {}, "bf16", True, True),
    ("standardised_history_1", a1_spec(1), a1(1, normalize=True), {"one_run_per_row": True}, "bf16", False, False),
    ("standardised_history_2", a1_spec(2), a1(2, normalize=True), {"one_run_per_row": True}, "bf16", True, True),
    ("standardised_history_256", a1_spec(256), a1(256, normalize=True), {}, "bf16", True, True),
    ("standardised_history_257", a1_spec(257), a1(257, normalize=True), {}, "bf16", False, False),
    ("unstandardised_history_257", a1_spec(257), a1(257), {}, "bf16", True, True),
    ("node_types_differ", A1, solo(), {}, "bf16", False, False),
    ("node_counts_differ", A1, a1(n_base=1), {}, "bf16", False, False),
    ("widths_differ", A1, a1(100), {}, "bf16", False, False),
    # training computes its loss from the recipe's labels; evaluation runs without them
    ("no_labels", A1, dataclasses.replace(a1(), label_cols=[]), {}, "bf16", False, True),
    # node rows of several runs need a history of 8: evaluation and the standardised training steps check it, the plain training steps do not
    ("several_runs_history_7", a1_spec(7), a1(7), {}, "bf16", True, False),
    ("several_runs_history_8", a1_spec(8), a1(8), {}, "bf16", True, True),
    ("several_runs_history_7_standardised", a1_spec(7), a1(7, normalize=True), {}, "bf16", False, False),
    ("several_runs_history_8_standardised", a1_spec(8), a1(8, normalize=True), {}, "bf16", True, True),
    ("one_run_per_row_history_7", a1_spec(7), a1(7), {"one_run_per_row": True}, "bf16", True, True),
    ("solo_history_1", SOLO, solo(1), {}, "bf16", True, False),
    # against a real Solo model (one time step) the widths already differ; with the widths matched, the several-runs check alone refuses, and only below a history of 8
    ("solo_history_2_standardised", SOLO, solo(2, normalize=True), {}, "bf16", False, False),
    ("solo_history_2_standardised_widths_matched", solo_spec(solo(2)), solo(2, normalize=True), {}, "bf16", False, False),
    ("solo_history_2_widths_matched", solo_spec(solo(2)), solo(2), {}, "bf16", True, False),
    ("solo_history_8_standardised_widths_matched", solo_spec(solo(8)), solo(8, normalize=True), {}, "bf16", True, True),
]


@pytest.mark.parametrize("spec,recipe,desc_kw,dtype,train,evaluate", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_window_route_rule(spec, recipe, desc_kw, dtype, train, evaluate):
    desc = desc_of(recipe, **desc_kw)
    assert _window_recipe_ok(spec, recipe, desc, dtype, training=True) is train
    assert _window_recipe_ok(spec, recipe, desc, dtype, training=False) is evaluate


def test_the_recipes_of_the_table_are_what_the_rows_say():
    """The several-runs rows rest on the real recipes' tables: A1 and Solo node rows hold several runs each."""
    for r in (a1(), solo()):
        d = desc_of(r)
        assert d.n_runs > d.n_rows
    for spec, r in ((A1, a1()), (SOLO, solo())):
        assert {t: r.width(t) for t in r.node_types} == spec.widths and list(r.node_types) == list(spec.node_types)
