"""Device field, bucket-point and saturated curve-point arithmetic, primitive by primitive, against Python integers
(tests/field_ref.py), with the operands at the top of the ranges their call sites declare and, for the XYZZ points of ec_dev.hpp,
at every exceptional case of the group law.  Each test runs one operation of the probe library (tests/hip/,
built by tests/field_probe.py) over all generated cases, one lane per case, and checks every row; nothing is filtered on the
device's answer.  A failure names the primitive: "fu-fu_sub_sel<2>-Bls381Fq", not "the 2^22 MSM differs".

Measured on an MI355X: the whole file (about 390 000 cases) takes 6 s; a device call is 0.1 to 1.2 ms, case generation and the
Python reference are the rest.  The 32 tests of the ec_dev.hpp operations ("ec-..."; 20 844 cases) add 2 s: a device call is
0.1 ms, the slowest test (ec2_add on Bls381Fq, 1584 cases) 0.12 s.
"""
import os
import time

import numpy as np
import pytest

from tests import field_probe
from tests import field_ref as R

pytestmark = pytest.mark.gpu

DEVICE = int(os.environ.get("ZKP_TEST_DEVICE", "0"))

# saturated operations run twice: fp_mul inlined (ZKP_INLINE_MUL) and out of line, the two forms the product's units use
PARAMS = []
for _op, _spec in R.OPS.items():
    for _f in _spec.fields:
        for _v in (("inl", "ool") if R.LAYER_OF[_op] == "fp" else ("",)):
            PARAMS.append(pytest.param(R.LAYER_OF[_op], _op, _f, _v, id="-".join(x for x in (R.LAYER_OF[_op], _op, _f, _v) if x)))


def run_cases(op, field, variant=""):
    spec, F = R.OPS[op], R.FIELDS[field]
    cases = R.make_cases(op, field)
    nin = max(len(c[0]) for c in cases)
    assert all(len(c[0]) == nin for c in cases)
    inp = np.array([c[0] for c in cases], dtype=np.uint32)
    nout = spec.nout(F)
    init = np.array([c[1] if c[1] is not None else [0xA5A5A5A5] * nout for c in cases], dtype=np.uint32)
    t0 = time.perf_counter()
    out = field_probe.run(DEVICE, (variant + ":" if variant else "") + op, field, inp, init)
    return spec, F, cases, out, time.perf_counter() - t0


@pytest.mark.parametrize("layer,op,field,variant", PARAMS)
def test_probe(layer, op, field, variant):
    spec, F, cases, out, dt = run_cases(op, field, variant)
    asserted = 0
    for (words, init, ctx), row in zip(cases, out):
        spec.check(F, ctx, row)
        asserted += 1
    print(f"{layer} {op} {field} {variant}: generated {len(cases)}, asserted {asserted}, device call {dt * 1e3:.1f} ms")
    assert asserted == len(cases)


@pytest.mark.parametrize("op,field", [(q, f) for q in R.QUAD_OF for f in R.OPS[q].fields])
def test_quad_equals_single_lane(op, field):
    """coop_dev.hpp: "the stored points are the same field elements" as BkPoint::add_mem / dbl_mem — limb for limb."""
    spec, F, cases, quad, _ = run_cases(op, field)
    _, _, cases1, single, _ = run_cases(R.QUAD_OF[op], field)
    assert [c[0] for c in cases] == [c[0] for c in cases1] and [c[1] for c in cases] == [c[1] for c in cases1]
    asserted = 0
    for (words, init, ctx), rq, rs in zip(cases, quad, single):
        a, b = spec.result(F, ctx, rq), spec.result(F, ctx, rs)
        assert np.array_equal(a, b), f"{op} [{ctx[0]}, out mode {ctx[2]}]: quad {list(a)} != single lane {list(b)}"
        asserted += 1
    print(f"{op} {field}: generated {len(cases)}, asserted {asserted}")
    assert asserted == len(cases)


def test_probe_rejects_unknown_operation():
    """An (op, field) the probe does not hold, or rows too short for the operation, launch nothing and say so."""
    one = np.zeros((1, 64), dtype=np.uint32)
    with pytest.raises(RuntimeError, match="-> -1"):
        field_probe.run(DEVICE, "no_such_op", "Bn254Fq", one, one)
    with pytest.raises(RuntimeError, match="-> -1"):
        field_probe.run(DEVICE, "quad_add_mem2", "Bls381Fq", one, one)
    with pytest.raises(RuntimeError, match="-> -2"):
        field_probe.run(DEVICE, "fu_mul", "Bn254Fq", one[:, :4], one)
