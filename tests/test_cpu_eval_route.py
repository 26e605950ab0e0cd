"""Truth table of gdn_amd.model.eval_route, the pure function that names the launches of an eval forward, and of the
launch table behind it.  Both tables below are written out by hand from the launch sequences the entry points had
before there was one dispatcher (DESIGN.md "Eval routes"); `ANY` stands for every value of a fact.  Every
combination of the facts must be claimed by exactly one row, so no row hides behind another."""
import itertools

from gdn_amd import model as M

W, S = M.WINDOWS, M.SERIES
ANY = None
KINDS, BOOLS, TAILS = (W, S), (False, True), (None, "plan", "wide")
HAS_TAIL = ("plan", "wide")

# (kind, bf16, mlp, large, planned, wide, guard, keys, tail) -> route or refusal
TABLE = [
    # out_layer_num > 1: staged at every shape, fp32 only, no keys, an OutLayer with a tail kernel
    ((ANY, ANY, True, ANY, ANY, ANY, ANY, True, ANY), "refuse_keys"),
    ((ANY, True, True, ANY, ANY, ANY, ANY, False, ANY), "refuse_bf16_mlp"),
    ((ANY, False, True, ANY, ANY, ANY, ANY, False, (None,)), "refuse_outlayer"),
    ((ANY, False, True, ANY, ANY, False, ANY, False, HAS_TAIL), "staged"),
    ((ANY, False, True, True, ANY, True, ANY, False, HAS_TAIL), "staged_wide"),
    ((S, False, True, False, ANY, True, ANY, False, HAS_TAIL), "staged_wide"),
    ((W, False, True, False, ANY, True, ANY, False, HAS_TAIL), "staged_wide_project"),    # gdn_project_fwd_wide: only here
    # out_layer_num == 1 beyond the LDS tile: staged, fp32 only, no keys
    ((ANY, ANY, False, True, ANY, ANY, ANY, True, ANY), "refuse_keys"),
    ((ANY, True, False, True, ANY, ANY, ANY, False, ANY), "refuse_bf16_shape"),
    ((ANY, False, False, True, ANY, False, ANY, False, ANY), "staged"),
    ((ANY, False, False, True, ANY, True, ANY, False, ANY), "staged_wide"),
    # out_layer_num == 1 on the tile, fp32
    ((ANY, False, False, False, ANY, True, ANY, True, ANY), "refuse_keys"),
    ((ANY, False, False, False, ANY, True, ANY, False, ANY), "gated"),
    ((ANY, False, False, False, False, False, ANY, True, ANY), "refuse_keys"),
    ((ANY, False, False, False, False, False, ANY, False, ANY), "tile"),                  # the guard is dropped
    ((ANY, False, False, False, True, False, ANY, True, ANY), "plan_keys"),
    ((ANY, False, False, False, True, False, True, False, ANY), "plan_guarded"),
    ((ANY, False, False, False, True, False, False, False, ANY), "plan"),
    # out_layer_num == 1 on the tile, bf16 storage: windows only; `wide` is ignored and the guard dropped
    ((S, True, False, False, ANY, ANY, ANY, ANY, ANY), "refuse_series_dtype"),
    ((W, True, False, False, False, ANY, ANY, True, ANY), "refuse_keys"),
    ((W, True, False, False, False, ANY, ANY, False, ANY), "tile_bf16"),
    ((W, True, False, False, True, ANY, ANY, True, ANY), "plan_keys"),
    ((W, True, False, False, True, ANY, ANY, False, ANY), "plan"),
]

# route -> C symbols in launch order for (windows, series); None: not launched from the table (the plan-less series
# form goes through ops.forward_fused_series, and eval_route never sends a series to the other two).  The head / MLP
# tail kernels that end a staged route follow these.
LAUNCHES = {
    "plan": (["gdn_forward_fused_plan"], ["gdn_forward_fused_series_plan"]),
    "plan_guarded": (["gdn_forward_fused_plan", "gdn_forward_fused_gated"],
                     ["gdn_forward_fused_series_plan", "gdn_forward_fused_series_gated"]),
    "plan_keys": (["gdn_forward_fused_plan_keys"], ["gdn_forward_fused_series_plan_keys"]),
    "gated": (["gdn_forward_fused_gated"], ["gdn_forward_fused_series_gated"]),
    "tile": (["gdn_forward_fused"], [None]),
    "tile_bf16": (["gdn_forward_fused_bf16"], [None]),
    "staged": (["gdn_project_fwd", "gdn_attn_aggregate_fwd"], ["gdn_project_fwd_series", "gdn_attn_aggregate_fwd"]),
    "staged_wide": (["gdn_project_fwd", "gdn_attn_aggregate_fwd_wide"],
                    ["gdn_project_fwd_series", "gdn_attn_aggregate_fwd_wide"]),
    "staged_wide_project": (["gdn_project_fwd_wide", "gdn_attn_aggregate_fwd_wide"], [None, "gdn_attn_aggregate_fwd_wide"]),
}


def _claims(pattern, facts):
    return all(p is ANY or (f in p if isinstance(p, tuple) else f == p) for p, f in zip(pattern, facts))


def test_every_combination_of_the_facts_has_its_route():
    combos = list(itertools.product(KINDS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, BOOLS, TAILS))
    assert len(combos) == 768
    for facts in combos:
        rows = [expected for pattern, expected in TABLE if _claims(pattern, facts)]
        assert len(rows) == 1, (facts, rows)
        assert M.eval_route(*facts) == rows[0], (facts, rows[0])


def test_launch_table_names_the_symbols_of_every_route():
    assert set(M._ROUTES) == set(LAUNCHES)
    assert {expected for _pattern, expected in TABLE if not expected.startswith("refuse_")} == set(LAUNCHES)
    for route, per_kind in LAUNCHES.items():
        for kind in KINDS:
            assert [M._SYMBOLS[step][kind] for step in M._ROUTES[route]] == per_kind[kind], (route, kind)
    from gdn_amd import _lib
    named = {s for pair in M._SYMBOLS.values() for s in pair if s is not None}
    assert named <= set(_lib.SIGNATURES)
