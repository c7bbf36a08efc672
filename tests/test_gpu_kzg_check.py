"""kzg10.check / kzg10.batch_check on the device: commit -> open -> check at degrees 1, 2 and 19 (19 is the reference's unit test,
marlin/src/pc/kzg10.rs:229-270), with and without blinding; a wrong value, a wrong point and a wrong witness are each rejected, and
the oracle's check agrees; batch_check over 1, 2 and 65 openings locates one bad opening by its index."""
import random

import pytest

from ckb_zkp_amd import codec, kzg10
from ckb_zkp_amd.params import get_curve
from oracle.pyref import kzg10 as okzg
from oracle.pyref.curves import Group
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
BETA = 0x123456789ABCDEF0123
MAX_DEGREE = 19


@pytest.fixture(scope="module", params=CURVES)
def key(request, ctx):
    curve = request.param
    ck = kzg10.setup(ctx, curve, MAX_DEGREE, BETA)
    yield curve, ck
    ck.powers_of_g.free()
    ck.powers_of_gamma_g.free()


def opening(ctx, ck, c, rng, degree, hiding):
    p = [rng.randrange(c.r) for _ in range(degree)] + [rng.randrange(1, c.r)]
    blind = [rng.randrange(c.r) for _ in range(3)] if hiding else None
    z = rng.randrange(c.r)
    pm = codec.fr_to_mont(p, c).reshape(-1, 4)
    bm = codec.fr_to_mont(blind, c).reshape(-1, 4) if hiding else None
    comm = kzg10.commit(ctx, ck, pm, bm)
    proof = kzg10.open(ctx, ck, pm, z, bm)
    return comm, z, okzg.evaluate(p, z, c.r), proof


@pytest.mark.parametrize("hiding", [False, True], ids=["plain", "blinded"])
@pytest.mark.parametrize("degree", [1, 2, 19])
def test_check(ctx, key, degree, hiding):
    curve, ck = key
    c = get_curve(curve)
    rng = random.Random(f"kzg-check-{curve}-{degree}-{hiding}")
    comm, z, v, (w, rand_v) = opening(ctx, ck, c, rng, degree, hiding)
    assert (rand_v is not None) == hiding
    assert kzg10.check(ctx, ck, comm, z, v, (w, rand_v)) is True
    assert kzg10.check(ctx, ck, comm, z, (v + 1) % c.r, (w, rand_v)) is False              # a wrong value
    assert kzg10.check(ctx, ck, comm, (z + 1) % c.r, v, (w, rand_v)) is False              # a wrong point
    G1 = Group(OC[curve], 1)
    assert kzg10.check(ctx, ck, comm, z, v, (G1.add(w, c.g1), rand_v)) is False            # a wrong witness
    if hiding:
        assert kzg10.check(ctx, ck, comm, z, v, (w, (rand_v + 1) % c.r)) is False
    if degree == 19:                                                                       # the oracle's check on the same opening
        pp = okzg.setup(OC[curve], MAX_DEGREE, BETA)
        assert okzg.check(pp, comm, z, v, w, rand_v)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batch_check(ctx, key, n):
    curve, ck = key
    c = get_curve(curve)
    rng = random.Random(f"kzg-batch-{curve}")
    base = [opening(ctx, ck, c, rng, d, h) for d, h in ((1, False), (2, True), (19, False), (7, True))]
    openings = [base[k % len(base)] for k in range(n)]
    assert kzg10.batch_check(ctx, ck, openings) == [True] * n
    bad = (2 * n) // 3
    comm, z, v, proof = openings[bad]
    openings[bad] = (comm, z, (v + 1) % c.r, proof)
    assert kzg10.batch_check(ctx, ck, openings) == [k != bad for k in range(n)]
