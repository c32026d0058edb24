"""Which kernel serves which forward / data-gradient pass, pinned: the plan functions of csrc/vf_conv.hip (ga_plan, tr_plan,
ig_plan) and csrc/vf_pgemm.hip (pg_plan) against a table recorded with the library as it was BEFORE they existed.

Every case of route_cases.CASES is one pass through HipBackend at one shape, product mode and workspace size, run under
prof_begin() / prof_end(); its launch names with their launch counts, flops and bytes (the bytes of a slab_reduce_* entry carry the
split count) must equal tests/golden/conv_routes.json, which `scripts/ab_conv_outputs.py record-routes` wrote from the parent
commit's library (VF_HIP_LIB, a fresh process).  The table names, per case, the enumerators of the route enums the case stands for;
every enumerator the sources declare is reached by at least one case.

What the launch names cannot tell, and this test therefore does not pin: IG_TILE_KLIN launches under the name an IG_TILE launch of
the 64 x 128 tile has (a mix-up of the two shows in the output bytes that scripts/ab_conv_outputs.py compares, and in the fp64
checks of the bottleneck forward in the suite); GA_DOT_HEAD, TR_DOT_HEAD and the pointwise bias pass behind TR_GEMM_1X1 are not
profiled under a name, so their cases pin only that no OTHER kernel is launched."""
import json

import pytest

import route_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    """a backend of its own: the cases re-point its workspace"""
    from video_filler_amd.backend import HipBackend
    b = HipBackend(workspace_bytes=1 << 20)
    yield b
    b.synchronize()


@pytest.fixture(scope="module")
def table():
    with open(RC.GOLDEN) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("c", RC.CASES, ids=lambda c: c["id"])
def test_pass_route_matches_the_recorded_table(c, rb, table):
    want = table[c["id"]]
    assert want["routes"] == c["routes"], "the table was recorded for other routes: record it again from the parent library"
    rec, _ = RC.run_case(rb, c)
    print(c["id"], rec)
    RC.check_routes(c, rec)
    assert rec == {n: list(v) for n, v in want["launches"].items()}


def test_every_route_enumerator_has_a_case(table):
    declared = RC.route_enumerators()
    assert len(declared) == len(set(declared)) and set(declared) == set(RC.ROUTE_NAMES), declared
    assert set(table) == set(c["id"] for c in RC.CASES)
    reached = set(r for c in RC.CASES for r in c["routes"])
    assert reached == set(declared), "no case for %s" % sorted(set(declared) - reached)
