"""Python-integer restatement of Libra's linear-time GKR, against the line numbers of libra/src/circuit.rs, evaluate.rs,
sumcheck.rs and libra_linear_gkr.rs.  Field elements are canonical integers mod r; no product imports.  The merlin transcript is
left out: `next_round(coeffs)` stands where the reference draws `challenge_nextround` after a round polynomial, `absorb_final(values)`
where it appends `claim_final`, `next_alpha_beta()` where it draws `challenge_alpha` / `challenge_beta`; the output point gu
(eval_output's challenges) is an argument."""
from tests.sumcheck_ref import combine_with_r, eval_eq, evaluate as poly_evaluate, quadratic_from_evals


class Layer:
    def __init__(self, gates_count, bit_size, gates):
        self.gates_count, self.bit_size, self.gates = gates_count, bit_size, gates    # gates: (g, op, left, right)


def _log2_ceil(n):
    return (n - 1).bit_length()


def input_new(num_inputs, num_aux):
    """Layer::input_new, circuit.rs:40-53"""
    gates_num = (1 << _log2_ceil(max(num_aux, num_inputs, 1))) * 2
    return Layer(gates_num, _log2_ceil(gates_num), [(g, 3, 0, 0) for g in range(gates_num)])


def mid_layer_new(gates_raw, next_layer_gates_count):
    """Layer::mid_layer_new, circuit.rs:55-80"""
    gates = []
    for g, (op, left, right) in enumerate(gates_raw):
        if op not in (0, 1):
            raise ValueError("IllegalOperator")
        if left >= next_layer_gates_count or right >= next_layer_gates_count:
            raise ValueError("IllegalNode")
        gates.append((g, op, left, right))
    return Layer(len(gates), _log2_ceil(len(gates)), gates)


class Circuit:
    """Circuit::new, circuit.rs:116-138"""

    def __init__(self, num_inputs, num_aux, layers_raw):
        self.layers = [input_new(num_inputs, num_aux)]
        for raw in layers_raw:
            self.layers.append(mid_layer_new(raw, self.layers[-1].gates_count))
        self.depth = len(self.layers)


def circuit_evaluate(circuit, inputs, aux, r):
    """Circuit::evaluate, circuit.rs:140-185"""
    evals = []
    for d, layer in enumerate(circuit.layers):
        if d == 0:
            input_size = 1 << (layer.bit_size - 1)
            assert input_size >= len(inputs) and input_size >= len(aux)
            values = [a % r for a in aux] + [0] * (input_size - len(inputs)) + [i % r for i in inputs] + [0] * (input_size - len(aux))
        else:
            below = evals[-1]
            values = [(below[left] * below[right] if op == 1 else below[left] + below[right]) % r for _, op, left, right in layer.gates]
        evals.append(values)
    return evals


def eval_layer(gates_raw, below, r):
    """one layer of circuit.rs:159-178 plus the zero padding of eval_output (evaluate.rs:16-21)"""
    out = [(below[left] * below[right] if op == 1 else below[left] + below[right]) % r for op, left, right in gates_raw]
    return out + [0] * ((1 << _log2_ceil(len(out))) - len(out))


def eval_value(value, rs, r):
    """evaluate.rs:72-76 (value may be shorter than 2^len(rs): the missing entries are zeros)"""
    return sum(v * e for v, e in zip(value, eval_eq(rs, r))) % r


def eval_output(output, bit_size, gu, r):
    """evaluate.rs:11-33 with the challenges given"""
    assert len(gu) == bit_size
    return eval_value(list(output) + [0] * ((1 << bit_size) - len(output)), gu, r)


def eval_hg(evals_g, v, gates, bit_size, r):
    """evaluate.rs:79-99"""
    mul, add1, add2 = ([0] * (1 << bit_size) for _ in range(3))
    for g, op, x, y in gates:
        if op == 1:
            mul[x] = (mul[x] + evals_g[g] * v[y]) % r
        elif op == 0:
            add1[x] = (add1[x] + evals_g[g]) % r
            add2[x] = (add2[x] + evals_g[g] * v[y]) % r
    return mul, add1, add2


def eval_fgu(evals_g, ru_vec, gates, bit_size, r):
    """evaluate.rs:101-119"""
    mul, add = ([0] * (1 << bit_size) for _ in range(2))
    for g, op, x, y in gates:
        if op == 1:
            mul[y] = (mul[y] + evals_g[g] * ru_vec[x]) % r
        elif op == 0:
            add[y] = (add[y] + evals_g[g] * ru_vec[x]) % r
    return mul, add


def eval_operators(layer, gu, gv, ru, rv, alpha, beta, r):
    """Layer::eval_operators, circuit.rs:82-108: (add_gate_eval, mult_gate_eval)"""
    eq_gu, eq_gv, eq_ru, eq_rv = (eval_eq(v, r) for v in (gu, gv, ru, rv))
    add = mul = 0
    for g, op, left, right in layer.gates:
        ev = (alpha * eq_gu[g] + beta * eq_gv[g]) * eq_ru[left] * eq_rv[right]
        if op == 0:
            add += ev
        elif op == 1:
            mul += ev
    return add % r, mul % r


def _g1(f, mul, add1, add2, r):
    return sum(a * b + a * c + d for a, b, c, d in zip(f, mul, add1, add2)) % r          # sumcheck.rs:44-48 (zip stops at size)


def _g2(f, mul, add, fu, r):
    return sum(m * a * fu + d * fu + d * a for a, m, d in zip(f, mul, add)) % r         # sumcheck.rs:120-126


def round_evals(phase, tables, fu, r):
    """g(0) and g(2) of one round over the given tables (phase 1: f, mul, add1, add2; phase 2: f, mul, add)"""
    size = len(tables[0]) // 2
    two = [combine_with_r(t, 2, r) for t in tables]
    if phase == 1:
        return _g1(*(t[:size] for t in tables), r), _g1(*two, r)
    return _g2(*(t[:size] for t in tables), fu, r), _g2(*two, fu, r)


def _phase(phase, tables, fu, claim, next_round, r):
    tables = [list(t) for t in tables]
    polys, rs = [], []
    for _ in range(len(tables[0]).bit_length() - 1):
        e0, e2 = round_evals(phase, tables, fu, r)                                         # :44-62 / :120-139
        e1 = (claim - e0) % r                                                              # :49
        poly = quadratic_from_evals(e0, e1, e2, r)                                         # :67-72: [c, b, a]
        x = next_round(list(poly)) % r                                                     # :74-77
        tables = [combine_with_r(t, x, r) for t in tables]                                 # :79-82
        claim = poly_evaluate(poly, x, r)                                                  # :84
        polys.append(poly)
        rs.append(x)
    return polys, rs, [t[0] for t in tables]


def phase_one_prover(f, g_vec, bit_size, claim, next_round, absorb_final, r):
    """SumCheckProof::phase_one_prover, sumcheck.rs:21-97: (polys, [f, mul, add1, add2] at ru, ru)"""
    assert all(len(t) == 1 << bit_size for t in (f, *g_vec))                              # :32-35
    polys, ru, finals = _phase(1, [f, *g_vec], None, claim, next_round, r)
    absorb_final(list(finals))                                                             # :89-90
    return polys, finals, ru


def phase_two_prover(f, g_vec, bit_size, claim, next_round, absorb_final, r):
    """SumCheckProof::phase_two_prover, sumcheck.rs:99-173: g_vec = (mul, add, fu); (polys, [f, mul, add] at rv, rv)"""
    mul, add, fu = g_vec
    assert all(len(t) == 1 << bit_size for t in (f, mul, add))                            # :109-111
    polys, rv, finals = _phase(2, [f, mul, add], fu, claim, next_round, r)
    absorb_final(list(finals))                                                             # :164-165
    return polys, finals, rv


def evals_g(gu, gv, alpha, beta, r):
    """libra_linear_gkr.rs:210-215"""
    return [(alpha * a + beta * b) % r for a, b in zip(eval_eq(gu, r), eval_eq(gv, r))]


def prove_layers(circuit, evals, gu, result_u, next_round, absorb_final, next_alpha_beta, r):
    """the loop of LinearGKRProof::prover, libra_linear_gkr.rs:38-110.
    Returns (proofs, ru, rv), proofs[i] = (polys_1, finals_1, polys_2, finals_2)"""
    alpha, beta = 1, 0
    gu = [x % r for x in gu]
    gv = [0] * len(gu)
    result_u, result_v = result_u % r, 0
    proofs, ru, rv = [], [], []
    for d in range(circuit.depth - 1, 0, -1):
        claim = (alpha * result_u + beta * result_v) % r                                   # :52
        uv_size = circuit.layers[d - 1].bit_size
        gates, v = circuit.layers[d].gates, evals[d - 1]
        g = evals_g(gu, gv, alpha, beta, r)
        polys_1, finals_1, ru = phase_one_prover(v, eval_hg(g, v, gates, uv_size, r), uv_size, claim, next_round, absorb_final, r)
        claim = (finals_1[0] * finals_1[1] + finals_1[0] * finals_1[2] + finals_1[3]) % r  # :72
        eq_ru = eval_eq(ru, r)
        fu = sum(a * b for a, b in zip(v, eq_ru)) % r                                      # :236
        mul, add = eval_fgu(g, eq_ru, gates, uv_size, r)
        polys_2, finals_2, rv = phase_two_prover(v, (mul, add, fu), uv_size, claim, next_round, absorb_final, r)
        proofs.append((polys_1, finals_1, polys_2, finals_2))
        if d > 1:                                                                          # :98-109
            gu, gv = list(ru), list(rv)
            result_u, result_v = fu, finals_2[0]
            alpha, beta = (x % r for x in next_alpha_beta())
    return proofs, ru, rv


def prover(circuit, inputs, aux, gu, next_round, absorb_final, next_alpha_beta, r):
    """LinearGKRProof::prover, libra_linear_gkr.rs:22-114: (proofs, output, evals, ru, rv)"""
    evals = circuit_evaluate(circuit, inputs, aux, r)
    result_u = eval_output(evals[-1], circuit.layers[-1].bit_size, gu, r)                  # :41-45
    proofs, ru, rv = prove_layers(circuit, evals, gu, result_u, next_round, absorb_final, next_alpha_beta, r)
    return proofs, evals[-1], evals, ru, rv


def verify(circuit, proofs, outputs, input_layer, gu, next_round, absorb_final, next_alpha_beta, r):
    """LinearGKRProof::verify, libra_linear_gkr.rs:116-198; input_layer: the values of layer 0.  A failed assert_eq of the
    reference is False here."""
    alpha, beta = 1, 0
    result_u, result_v = eval_output(outputs, circuit.layers[-1].bit_size, gu, r), 0      # :125-129
    if len(proofs) != circuit.depth - 1:                                                   # :135
        return False
    ru_vec, rv_vec, eval_ru_x, eval_rv_y = [], [], 0, 0
    for d, (polys_1, finals_1, polys_2, finals_2) in enumerate(proofs):
        claim = (alpha * result_u + beta * result_v) % r                                   # :137
        bit_size = circuit.layers[circuit.depth - d - 2].bit_size
        if len(polys_1) != bit_size or len(polys_2) != bit_size:
            return False
        ru_vec, rv_vec = [], []
        for poly in polys_1:                                                               # :143-155
            if (poly_evaluate(poly, 0, r) + poly_evaluate(poly, 1, r)) % r != claim:
                return False
            x = next_round(list(poly)) % r
            ru_vec.append(x)
            claim = poly_evaluate(poly, x, r)
        absorb_final(list(finals_1))                                                       # :157
        if claim != (finals_1[0] * finals_1[1] + finals_1[0] * finals_1[2] + finals_1[3]) % r:   # :158-161
            return False
        for poly in polys_2:                                                               # :162-174
            if (poly_evaluate(poly, 0, r) + poly_evaluate(poly, 1, r)) % r != claim:
                return False
            x = next_round(list(poly)) % r
            rv_vec.append(x)
            claim = poly_evaluate(poly, x, r)
        absorb_final(list(finals_2))                                                       # :176
        if claim != (finals_2[1] * finals_2[0] * finals_1[0] + finals_2[2] * finals_1[0] + finals_2[2] * finals_2[0]) % r:   # :177-180
            return False
        if d < circuit.depth - 2:                                                          # :181-189
            result_u, result_v = finals_1[0], finals_2[0]
            alpha, beta = (x % r for x in next_alpha_beta())
        else:
            eval_ru_x, eval_rv_y = finals_1[0], finals_2[0]
    return eval_ru_x == eval_value(input_layer, ru_vec, r) and eval_rv_y == eval_value(input_layer, rv_vec, r)   # :195-197
