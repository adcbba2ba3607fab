"""tests/f64_judge.py on the CPU: the rules every float64 suite leans on, pinned directly on synthetic tensors of a few dozen elements,
through the three callers that parameterise them (step_f64_oracle.judge, glue_f64_oracle.judge, util.assert_close_vs_f64).

The yardstick is 0 everywhere and every scale a power of two, so a result IS its error times the scale, exactly: "exactly at the
bound" and "the next float64 above it" are exact statements, and no tolerance appears in this file."""
import json
import math

import numpy as np
import pytest
import torch

from tests import f64_judge as J
from tests import glue_f64_oracle as G
from tests import step_f64_oracle as S
from tests.util import assert_close_vs_f64

F64 = torch.float64
N = 64
INF = math.inf
REL_FLOOR = 2.0 ** -10          # assert_close_vs_f64's `floor`: with a yardstick of 0 it is every element's scale


def up(x):
    return math.nextafter(x, INF)


def _step(hip, ref, f64, scale):
    return S.judge(hip, ref, f64, scale, "t")


def _glue(hip, ref, f64, scale):
    return G.judge(hip, ref, f64, scale, 4, "t")


def _util(hip, ref, f64, scale):
    assert bool((J.flat64(scale) == REL_FLOOR).all())
    return assert_close_vs_f64(hip, ref, f64, "t", floor=REL_FLOOR)


# name -> (caller, factor, floor of the worst-error rule, scale of every element)
RULES = {"step": (_step, 2.0, S.FLOOR_ULPS * J.U, 0.5), "glue": (_glue, 3.0, 4 * J.U, 0.5), "util": (_util, 2.0, 1e-4, REL_FLOOR)}
R = 2.0 ** -8                   # a restatement error far above every floor


def _inputs(rule, e_hip, e_ref, n=N):
    """-> (hip, ref, f64, scale): yardstick 0, the listed errors in the first elements, exact elsewhere"""
    scale = RULES[rule][3]
    hip, ref = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    hip[:len(e_hip)] = torch.tensor(e_hip, dtype=F64) * scale
    ref[:len(e_ref)] = torch.tensor(e_ref, dtype=F64) * scale
    return hip, ref, torch.zeros(n, dtype=F64), torch.full((n,), scale, dtype=F64)


def _judge(rule, e_hip, e_ref, n=N):
    return RULES[rule][0](*_inputs(rule, e_hip, e_ref, n))


@pytest.mark.parametrize("rule", list(RULES))
def test_worst_error_at_factor_times_the_restatement(rule):
    factor = RULES[rule][1]
    _judge(rule, [factor * R], [R / 2, R])
    with pytest.raises(AssertionError, match="worst error"):
        _judge(rule, [up(factor * R)], [R / 2, R])


@pytest.mark.parametrize("rule", list(RULES))
def test_exact_restatement_holds_the_kernel_to_the_floor(rule):
    floor = RULES[rule][2]
    _judge(rule, [floor], [])
    with pytest.raises(AssertionError, match="worst error"):
        _judge(rule, [up(floor)], [])


@pytest.mark.parametrize("rule", ["step", "util"])
def test_count_above_the_floor(rule):
    """three restatement elements above the floor allow int(2 x 3) + 2 = 8; elements exactly AT the floor are not above it"""
    floor = RULES[rule][2]
    at_floor = [floor] * 20
    _judge(rule, [R] * 8 + at_floor, [R] * 3 + at_floor)
    with pytest.raises(AssertionError, match="9 elements above"):
        _judge(rule, [R] * 9 + at_floor, [R] * 3 + at_floor)
    _judge(rule, [up(floor)] * 2, [floor])                 # no restatement element above the floor: the slack alone
    with pytest.raises(AssertionError, match="3 elements above"):
        _judge(rule, [up(floor)] * 3, [floor])


def test_glue_counts_above_the_percentile_not_the_floor():
    """64 elements, the restatement's two largest errors R / 2 and R: the 99.9th percentile lies between them, far above the floor.
    One restatement element is above it: 3 x 1 + 2 = 5 kernel elements may be.  Twenty kernel elements at R / 2 are above the floor
    and below the percentile: the floor as threshold would count them and fail."""
    f = J.judge_vs_f64(*_inputs("glue", [R] * 5, [R / 2, R]), "t", 3.0, 4 * J.U, 2, percentile=True)
    assert R / 2 < f["threshold"] < R and f["threshold"] > 1000 * 4 * J.U and (f["n_hip"], f["n_ref"]) == (5, 1)
    between = [R / 2] * 20
    assert _judge("glue", [R] * 5 + between, [R / 2, R])["n_above"] == 5
    with pytest.raises(AssertionError, match="6 elements above"):
        _judge("glue", [R] * 6 + between, [R / 2, R])
    with pytest.raises(AssertionError, match="25 elements above"):
        J.judge_vs_f64(*_inputs("glue", [R] * 5 + between, [R / 2, R]), "t", 3.0, 4 * J.U, 2)      # the floor as threshold
    # where the floor is the larger of the two it decides; no restatement element above it: the slack alone
    floor = 4 * J.U
    assert _judge("glue", [up(floor)] * 2 + [floor] * 20, [floor])["n_above"] == 2
    with pytest.raises(AssertionError, match="3 elements above"):
        _judge("glue", [up(floor)] * 3 + [floor] * 20, [floor])


def test_glue_single_element_takes_the_worst_as_threshold():
    f = J.judge_vs_f64(*_inputs("glue", [3 * R], [R], n=1), "t", 3.0, 4 * J.U, 2, percentile=True)
    assert f == dict(worst_hip=3 * R, worst_ref=R, n_hip=1, n_ref=0, threshold=R, n=1, bad_hip=0, bad_ref=0)
    assert _judge("glue", [3 * R], [R], n=1) == dict(worst_hip=3 * R, worst_chain=R, ratio=3.0, n_above=1)
    with pytest.raises(AssertionError, match="worst error"):
        _judge("glue", [up(3 * R)], [R], n=1)


@pytest.mark.parametrize("rule", ["step", "glue"])
def test_zero_scale_elements_must_be_exact(rule):
    call = RULES[rule][0]
    hip, ref, f64, scale = _inputs(rule, [R], [R])
    scale[5] = 0.0
    call(hip, ref, f64, scale)
    off = hip.clone()
    off[5] = 2.0 ** -60
    with pytest.raises(AssertionError, match="zero scale"):
        call(off, ref, f64, scale)
    ref_off = ref.clone()
    ref_off[5] = 2.0 ** -60
    if rule == "step":                                     # the restatement's own zero-scale elements: asserted by the step rule only
        with pytest.raises(AssertionError, match="zero scale"):
            call(hip, ref_off, f64, scale)
    else:
        call(hip, ref_off, f64, scale)
    assert J.scaled_errors(off, f64, scale)[1] == 1 and J.scaled_errors(off, f64, scale)[0].numel() == N - 1


@pytest.mark.parametrize("bad", [math.nan, INF, -INF])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("rule", list(RULES))
def test_non_finite_input_fails(rule, which, bad):
    args = list(_inputs(rule, [R], [R]))
    RULES[rule][0](*args)
    args[which] = args[which].clone()
    args[which][7] = bad
    with pytest.raises(AssertionError, match="finite"):
        RULES[rule][0](*args)


def test_records(monkeypatch, tmp_path, capsys):
    f = J.judge_vs_f64(*_inputs("step", [R], [R / 2]), "t", 2.0, 4 * J.U, 2)
    assert f == dict(worst_hip=R, worst_ref=R / 2, n_hip=1, n_ref=1, threshold=4 * J.U, n=N, bad_hip=0, bad_ref=0)
    # step: printed, reported and returned, the report written before anything is asserted
    path = tmp_path / "sub" / "step.jsonl"
    monkeypatch.setenv("MORPHEUS_STEP_REPORT", str(path))
    rec = _judge("step", [R], [R / 2])
    assert rec == dict(what="t", worst_hip=R, worst_ref=R / 2, ratio=2.0, n_hip=1, n_ref=1, n=N, factor=2.0)
    assert capsys.readouterr().out.startswith("[step-f64] t: kernel ")
    assert _judge("step", [J.U], [])["ratio"] is None, "an exact restatement: no ratio"
    with pytest.raises(AssertionError):
        _judge("step", [4 * R], [R])
    lines = [json.loads(line) for line in path.read_text().splitlines()]
    assert lines[0] == rec and len(lines) == 3 and lines[2]["worst_hip"] == 4 * R
    # glue: the ratio is taken against max(the chain's worst, floor); nothing live: the early return
    assert _judge("glue", [R], [R / 2]) == dict(worst_hip=R, worst_chain=R / 2, ratio=2.0, n_above=1)
    assert _judge("glue", [2 * J.U], []) == dict(worst_hip=2 * J.U, worst_chain=0.0, ratio=0.5, n_above=0)
    z = torch.zeros(3, dtype=F64)
    assert G.judge(z, z, z, 0.0, 0, "t") == dict(worst_hip=0.0, worst_chain=0.0, ratio=0.0, n_above=0)
    # a scalar scale is every element's, and a Python float is not rounded to fp32 on the way
    assert G.judge(z + 0.1, z + 0.1, z, 0.1, 1, "t")["worst_hip"] == 1.0
    # util: (worst_hip, n_hip, worst_ref, n_ref); above the floor the scale is |f64|
    assert _judge("util", [R, R], [R / 2]) == (R, 2, R / 2, 1)
    f64 = torch.full((4,), 4.0, dtype=F64)
    assert assert_close_vs_f64(f64 + 4 * R, f64 + 2 * R, f64, "t", floor=REL_FLOOR) == (R, 4, R / 2, 4)


def test_judge_sum():
    z, one = torch.zeros(2, dtype=F64), torch.tensor([1.0, 0.0], dtype=F64)
    at = torch.tensor([3 * J.U, 0.0], dtype=F64)
    assert G.judge_sum is J.judge_sum
    assert J.judge_sum(at, z, one, 3, "t") == dict(worst_hip=3 * J.U, worst_chain=None, ratio=1.0, n_above=0)
    with pytest.raises(AssertionError, match="bound"):
        J.judge_sum(torch.tensor([up(3 * J.U), 0.0], dtype=F64), z, one, 3, "t")
    with pytest.raises(AssertionError, match="exactly 0"):
        J.judge_sum(torch.tensor([0.0, 2.0 ** -100], dtype=F64), z, one, 3, "a sum without terms")
    extra = 2.0 ** -30
    assert J.judge_sum(at + extra, z, one, 3, "t", extra=extra)["ratio"] == 1.0
    with pytest.raises(AssertionError):
        J.judge_sum(at + extra, z, one, 3, "t")
    with pytest.raises(AssertionError, match="non-finite"):
        J.judge_sum(torch.tensor([math.nan, 0.0], dtype=F64), z, one, 3, "t")


def test_within_four_corners():
    floor = 2.0 ** -22
    assert J.within(3 * R, R, 3.0, floor) and not J.within(up(3 * R), R, 3.0, floor)              # the factor decides
    assert J.within(floor, floor / 8, 3.0, floor) and not J.within(up(floor), floor / 8, 3.0, floor)      # the floor decides
    assert J.within(floor, 0.0, 3.0, floor) and not J.within(up(floor), 0.0, 3.0, floor)
    assert J.within(0.0, 0.0, 3.0, 0.0) and not J.within(math.nan, R, 3.0, floor)


def test_report_and_append(monkeypatch, tmp_path):
    monkeypatch.delenv("MORPHEUS_TEST_REPORT", raising=False)
    J.report("MORPHEUS_TEST_REPORT", dict(a=1))
    assert list(tmp_path.iterdir()) == []
    path = tmp_path / "made" / "on" / "demand.jsonl"
    monkeypatch.setenv("MORPHEUS_TEST_REPORT", str(path))
    J.report("MORPHEUS_TEST_REPORT", dict(a=1, b=None, c=0.5))
    assert [json.loads(line) for line in path.read_text().splitlines()] == [dict(a=1, b=None, c=0.5)]
    J.append_jsonl(str(path), dict(a=2))
    assert [json.loads(line)["a"] for line in path.read_text().splitlines()] == [1, 2]
    J.append_jsonl(str(path / "below_a_file.jsonl"), dict(a=3))      # cannot be created: swallowed
    assert len(path.read_text().splitlines()) == 2


def test_flat64():
    for t, want in ((np.arange(6, dtype=np.float32).reshape(2, 3), list(range(6))), (1.5, [1.5]), (3, [3.0]),
                    (torch.arange(4.0).reshape(2, 2).requires_grad_(True), [0.0, 1.0, 2.0, 3.0]), (torch.tensor(2.0, dtype=torch.float16), [2.0])):
        f = J.flat64(t)
        assert f.dtype == F64 and f.dim() == 1 and f.device.type == "cpu" and not f.requires_grad and f.tolist() == want
    assert J.U == 2.0 ** -24 and float(np.float32(1) + np.float32(J.U)) == 1.0 and float(np.float32(1) + np.float32(2 * J.U)) > 1.0
