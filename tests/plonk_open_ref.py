"""REFERENCE (test infrastructure only): what Plonk::prove (plonk/src/lib.rs:93-204) does after round 3, in Python integers: the
coefficient table, the evaluations of AHPForPLONK::construct_linear_combinations (ahp/mod.rs:29-113) at verifier_query_set
(ahp/verifier.rs:77-99), the terms of the linearisation polynomial r (indexer/arithmetic.rs:22-38, indexer/permutation.rs:32-65),
verifier_equality_check (verifier.rs:101-150) and the two opening polynomials by synthetic division.  Builds on
tests/plonk_ref.py; nothing here shares code with ckb_zkp_amd/plonk.py."""
import json
from pathlib import Path

from tests import plonk_ref as ref
from tests.plonk_cases import KS, MINI_CHALLENGES, mini_circuit

GOLDEN = Path(__file__).resolve().parent / "golden" / "plonk_open_mini.json"
MINI_ZETA = 0x7A6574615F6D696E695F706C6F6E6B5F6F70656E
MINI_EPSILON = 0x657073696C6F6E5F31323334353637383930
PROVER = ("w_0", "w_1", "w_2", "w_3", "z", "t_0", "t_1", "t_2", "t_3")          # AHPForPLONK::LABELS
BASE = PROVER + ref.Q_NAMES + ref.S_NAMES                                       # the 20 polynomials of n coefficients
LABELS = ("q_arith", "r", "sigma_0", "sigma_1", "sigma_2", "t", "w_0", "w_1", "w_2", "w_3", "z")   # lib.rs:171-183: sorted
AT_ZETA = tuple(k for k in LABELS if k != "z")                                  # the ten labels queried at zeta


def coeff_table(ix, polys):
    """name -> n coefficients for the 20 base polynomials: prove_rounds' output and the interpolated selectors"""
    table = {k: list(polys[k]) for k in PROVER}
    for name in ref.Q_NAMES + ref.S_NAMES:
        table[name] = ix.dn.ifft(ix.sel[name])
    assert all(len(v) == ix.n for v in table.values())
    return table


def base_evals(ix, table, zeta):
    """the 20 polynomials at zeta and z at zeta w ("z_shifted")"""
    r = ix.r
    ev = {k: ref.horner(table[k], zeta, r) for k in BASE}
    ev["z_shifted"] = ref.horner(table["z"], zeta * ix.dn.group_gen % r, r)
    return ev


def first_lagrange(n, zeta, r):
    """evaluate_first_lagrange_poly (utils.rs:45-50)"""
    return (pow(zeta, n, r) - 1) * pow(n * (zeta - 1), -1, r) % r


def linearisation_terms(ix, ev, beta, gamma, alpha, zeta):
    """the eight (scalar, label) terms of r: arithmetic.rs:22-38 then permutation.rs:32-65, signs as written there"""
    r, ks = ix.r, ix.ks
    w = [ev[f"w_{j}"] for j in range(4)]
    qa = ev["q_arith"]
    terms = [(qa * w[0] % r, "q_0"), (qa * w[1] % r, "q_1"), (qa * w[2] % r, "q_2"), (qa * w[3] % r, "q_3"),
             (qa * w[1] * w[2] % r, "q_m"), (qa, "q_c")]
    num = den = 1
    for j in range(4):
        num = num * (w[j] + ks[j] * beta * zeta + gamma) % r
    for j in range(3):
        den = den * (w[j] + beta * ev[f"sigma_{j}"] + gamma) % r
    den = den * beta * ev["z_shifted"] % r
    l1 = first_lagrange(ix.n, zeta, r)
    terms.append(((num * alpha + l1 * alpha * alpha) % r, "z"))
    terms.append((-den * alpha % r, "sigma_3"))
    return terms


def lc_evals(ix, ev, terms, zeta):
    """the eleven evaluations in the reference's order (LABELS); z is the one at zeta w"""
    r = ix.r
    zn = pow(zeta, ix.n, r)
    out = {k: ev[k] for k in ("q_arith", "sigma_0", "sigma_1", "sigma_2", "w_0", "w_1", "w_2", "w_3")}
    out["z"] = ev["z_shifted"]
    out["t"] = sum(pow(zn, k, r) * ev[f"t_{k}"] for k in range(4)) % r
    out["r"] = sum(s * ev[label] for s, label in terms) % r
    return {k: out[k] for k in LABELS}


def pi_at(ix, public_inputs, zeta):
    """pi(zeta) in Lagrange form over the non-zero public inputs: sum pi_i w^i (zeta^n - 1) / (n (zeta - w^i))"""
    r, n = ix.r, ix.n
    zn1 = (pow(zeta, n, r) - 1) % r
    acc = 0
    for i, v in enumerate(public_inputs):
        if v % r:
            wi = ix.roots[i]
            acc += v * wi % r * zn1 % r * pow(n * (zeta - wi), -1, r)
    return acc % r


def equality_check(ix, evals, public_inputs, beta, gamma, alpha, zeta):
    """verifier_equality_check (verifier.rs:101-150)"""
    r = ix.r
    v_zeta = (pow(zeta, ix.n, r) - 1) % r
    pi_zeta = pi_at(ix, public_inputs, zeta)
    l1 = first_lagrange(ix.n, zeta, r)
    lhs = evals["t"] * v_zeta % r
    prod = evals["z"]
    for j in range(3):
        prod = prod * (evals[f"w_{j}"] + beta * evals[f"sigma_{j}"] + gamma) % r
    prod = prod * (evals["w_3"] + gamma) % r
    rhs = (evals["r"] + evals["q_arith"] * pi_zeta - prod * alpha - l1 * alpha * alpha) % r
    return lhs == rhs


def lincomb(terms, table, n, r):
    """the polynomial of a LinearCombination: sum scalar * table[label], n coefficients"""
    out = [0] * n
    for s, label in terms:
        for i, c in enumerate(table[label]):
            out[i] = (out[i] + s * c) % r
    return out


def div_linear(p, z, r):
    """synthetic division: p = q (X - z) + rem -> (q of len(p) - 1 coefficients, rem)"""
    q, acc = [0] * (len(p) - 1), 0
    for i in range(len(p) - 1, 0, -1):
        acc = (p[i] + acc * z) % r
        q[i - 1] = acc
    return q, (p[0] + acc * z) % r


def zeta_terms(ix, terms, weights, zeta):
    """sum_label weights[label] LC_label over the ten labels queried at zeta, expanded into (scalar, base polynomial) terms: the
    LCs t and r contribute their terms, so every one of the 20 base polynomials appears exactly once"""
    r = ix.r
    zn = pow(zeta, ix.n, r)
    acc = {k: 0 for k in BASE}
    for label in AT_ZETA:
        wgt = weights[label] % r
        if label == "t":
            for k in range(4):
                acc[f"t_{k}"] += wgt * pow(zn, k, r)
        elif label == "r":
            for s, name in terms:
                acc[name] += wgt * s
        else:
            acc[label] += wgt
    return [(acc[k] % r, k) for k in BASE]


def opening_polys(ix, table, terms, evals, weights, zeta):
    """((W_zeta, its remainder, the combined polynomial, the combined value), (W_shifted_zeta, remainder)): W_zeta =
    (sum_label weights[label] LC_label) / (X - zeta), W_shifted_zeta = z / (X - zeta w)"""
    r = ix.r
    comb = lincomb(zeta_terms(ix, terms, weights, zeta), table, ix.n, r)
    v = sum(weights[k] * evals[k] for k in AT_ZETA) % r
    wz, rem = div_linear(comb, zeta, r)
    ws, rem_s = div_linear(table["z"], zeta * ix.dn.group_gen % r, r)
    return (wz, rem, comb, v), (ws, rem_s)


def epsilon_weights(epsilon, r):
    """epsilon^j over the labels queried at zeta in ascending order, from epsilon^0"""
    return {k: pow(epsilon, j, r) for j, k in enumerate(AT_ZETA)}


def run(ix, polys, public_inputs, beta, gamma, alpha, zeta, weights):
    """everything after round 3 for the polynomials `polys` of prove_rounds"""
    table = coeff_table(ix, polys)
    ev = base_evals(ix, table, zeta)
    terms = linearisation_terms(ix, ev, beta, gamma, alpha, zeta)
    evals = lc_evals(ix, ev, terms, zeta)
    (wz, rem, comb, v), (ws, rem_s) = opening_polys(ix, table, terms, evals, weights, zeta)
    return {"table": table, "base": ev, "terms": terms, "evals": evals, "r_poly": lincomb(terms, table, ix.n, ix.r), "w_zeta": wz,
            "w_zeta_rem": rem, "combined": comb, "combined_value": v, "w_shifted": ws, "w_shifted_rem": rem_s}


def make_golden():
    """the content of tests/golden/plonk_open_mini.json: the mini circuit on BLS12-381 with MINI_CHALLENGES, MINI_ZETA, MINI_EPSILON"""
    cs = mini_circuit(ref.RefComposer("bls12_381"))
    ix = ref.RefIndex(cs, KS)
    ch = (MINI_CHALLENGES["beta"], MINI_CHALLENGES["gamma"], MINI_CHALLENGES["alpha"])
    polys = ref.prove_rounds(ix, cs.synthesize(), cs.public_inputs(), *ch)
    assert polys["closes"]
    out = run(ix, polys, cs.public_inputs(), *ch, MINI_ZETA % ix.r, epsilon_weights(MINI_EPSILON, ix.r))
    return {"curve": "bls12_381", "n": ix.n, "zeta": str(MINI_ZETA), "epsilon": str(MINI_EPSILON),
            "evaluations": {k: str(v) for k, v in out["evals"].items()},
            "r_terms": [[str(s), label] for s, label in out["terms"]],
            "w_zeta": [str(v) for v in out["w_zeta"]], "w_shifted_zeta": [str(v) for v in out["w_shifted"]]}


def load_golden():
    return json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps(make_golden(), indent=1) + "\n")
