"""Host side of the NTT variant tests (tests/ntt_variant_child.py) without a GPU: the pass plans behind the variant table, the
count a parent expects from a spec, the child's loop against a stand-in whose transforms are the oracle's own answers, and what the
parent does with a child that died, skipped work or reported a mismatch."""
import json
import sys

import pytest

from oracle import cpu_oracle
from tests import ntt_variant_child as nv


def test_pass_plans_of_the_variant_table():
    assert [nv.plan(k) for k in (1, 9, 10, 16, 17, 18, 19, 20)] == [[1], [9], [5, 5], [8, 8], [9, 8], [9, 9], [7, 6, 6], [7, 7, 6]]
    assert [nv.plan(k, 4) for k in (5, 8, 9, 12, 13, 16, 17)] == \
        [[3, 2], [4, 4], [3, 3, 3], [4, 4, 4], [4, 3, 3, 3], [4, 4, 4, 4], [4, 4, 3, 3, 3]]
    assert [nv.plan(k, 7) for k in (8, 14, 15, 18)] == [[4, 4], [7, 7], [5, 5, 5], [6, 6, 6]]
    assert [nv.plan(k, 10) for k in (10, 19)] == [[10], [10, 9]]
    assert nv.smax_of({}) == 9 and nv.smax_of({"ZKP_NTT_SMAX": "3"}) == 4 and nv.smax_of({"ZKP_NTT_SMAX": "12"}) == 10


def test_unit_positions_sit_on_the_first_tile_rows():
    assert nv.unit_positions(0) == [] and nv.unit_positions(15) == []
    assert nv.unit_positions(1) == [0, 1] and nv.unit_positions(9) == [0, 1, 511]          # one pass: rows are 1 apart
    assert nv.unit_positions(12) == [1, 63, 64, 4095]                                       # 6 + 6
    assert nv.unit_positions(9, 4) == [1, 63, 64, 511] and nv.unit_positions(13, 4) == [1, 511, 512, 8191]


def test_expected_counts():
    assert nv.expected_checked({"ntt": [], "witness": [4, 9, 12]}) == 6
    assert nv.expected_checked({"ntt": [0, 19]}) == 2 * 4 * (3 + 3)                          # dense inputs only
    assert nv.expected_checked({"ntt": [9], "witness": [9]}) == 2 * (4 * 6 + 1)
    assert nv.expected_checked({"ntt": [9], "witness": [9]}, smax=4) == 2 * (4 * 7 + 1)
    assert len(nv.VARIANTS) == 12 and len({v[0] for v in nv.VARIANTS}) == 12


class _OracleAsDevice:
    """stands in for Context: ntt returns the oracle's own answer"""

    def ntt(self, curve, x, op):
        return cpu_oracle.ntt(nv.CURVES.index(curve), x, op)


@pytest.mark.parametrize("variant", nv.VARIANTS, ids=[v[0] for v in nv.VARIANTS])
def test_child_loop_counts_what_the_parent_expects(variant):
    """the `ntt` half of every spec (sizes up to 2^8 here), run against the stand-in: no mismatch, and exactly the expected count"""
    _, switches, log_ns, _ = variant
    spec = {"ntt": [k for k in log_ns if k <= 8]}
    res = nv.run_spec(_OracleAsDevice(), cpu_oracle, spec, nv.smax_of(switches))
    assert res == {"checked": nv.expected_checked(spec, nv.smax_of(switches)), "mismatches": []}


def test_child_loop_reports_the_first_bad_index():
    class Wrong(_OracleAsDevice):
        def ntt(self, curve, x, op):
            y = super().ntt(curve, x, op)
            if op == 2:
                y[5, 0] ^= 1
            return y
    res = nv.run_spec(Wrong(), cpu_oracle, {"ntt": [3]}, 9)
    assert res["checked"] == nv.expected_checked({"ntt": [3]})
    assert len(res["mismatches"]) == 2 * len(nv.input_names(3)) and res["mismatches"][0] == ["bn254", "uniform", 3, 2, 5]


def _stand_in(code):
    return [sys.executable, "-c", code]


SPEC = {"ntt": [], "witness": [4]}
GOOD = json.dumps({"checked": 2, "mismatches": []})


def test_parent_accepts_only_a_complete_clean_answer(monkeypatch):
    monkeypatch.setattr(nv, "gpu_dead", None)
    assert nv.run_variant({}, SPEC, _stand_in(f"print('noise'); print('{GOOD}')"))["checked"] == 2
    for answer in ({"checked": 1, "mismatches": []}, {"checked": 2, "mismatches": [["bn254", "witness", 4, -1, 0]]}):
        with pytest.raises(AssertionError):
            nv.run_variant({}, SPEC, _stand_in(f"print('{json.dumps(answer)}')"))
    with pytest.raises(AssertionError):                                    # a failed child that printed a clean answer
        nv.run_variant({}, SPEC, _stand_in(f"print('{GOOD}'); raise SystemExit(1)"))
    with pytest.raises(AssertionError):
        nv.run_variant({}, SPEC, _stand_in("pass"))
    assert nv.gpu_dead is None                                             # none of these is a dead child


@pytest.mark.parametrize("code", ["import os, signal; os.kill(os.getpid(), signal.SIGKILL)", "raise SystemExit(134)",
                                  "raise SystemExit(139)", "raise SystemExit(124)", "raise SystemExit(137)",
                                  f"print('{GOOD}'); print('HIP error: an illegal memory access was encountered')"],
                         ids=["signal", "134", "139", "124", "137", "illegal-access"])
def test_a_dead_child_stops_the_later_cases(monkeypatch, tmp_path, code):
    monkeypatch.setattr(nv, "gpu_dead", None)
    with pytest.raises(AssertionError):
        nv.run_variant({"ZKP_NTT_V2": "0"}, SPEC, _stand_in(code))
    assert nv.gpu_dead and "ZKP_NTT_V2" in nv.gpu_dead
    mark = tmp_path / "started"
    with pytest.raises(AssertionError, match="not started"):
        nv.run_variant({}, SPEC, _stand_in(f"open({str(mark)!r}, 'w').close(); print('{GOOD}')"))
    assert not mark.exists()
