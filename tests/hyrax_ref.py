"""Python-integer restatement of Hyrax's data-parallel GKR, against the line numbers of hyrax/src/zk_sumcheck_proof.rs,
hyrax_proof.rs, evaluate.rs and circuit.rs.  Field elements are canonical integers mod r; no product imports.  Commitments, blinds
and the merlin transcript are left out: `next_round(coeffs)` stands where the reference draws `challenge_nextround` after a round
polynomial, `next_u()` where it draws u0 / u1; the output points (q', q) of eval_outputs are arguments.

Two provers of one layer: `sumcheck_literal` keeps the reference's tables (the G x n temp_vec, the per-gate ng-element left_eq /
right_eq vectors) and walks them as it does; `sumcheck_fast` uses the rank-one form of temp_vec and Libra's bookkeeping tables
(tests/gkr_ref.py).  tests/test_hyrax_ref.py pins one to the other.  Circuits are tests/gkr_ref.Circuit (layer 0 = the inputs);
a layer over all copies is a list of rows, rows[node][copy]."""
from tests import gkr_ref
from tests.sumcheck_ref import combine_with_r, cubic_from_evals, eval_eq, eval_eq_x_y, evaluate as poly_evaluate, quadratic_from_evals


def convert_to_bit(i, log_g):
    """evaluate.rs:237-251: the bits of i, top bit first"""
    return [(i >> (log_g - 1 - b)) & 1 for b in range(log_g)]


def _op(op, a, b):
    return a * b if op == 1 else a + b


def circuit_evaluate_batch(circuit, inputs, witnesses, r):
    """Circuit::evaluate per copy (circuit.rs:115-163), regrouped as hyrax_proof.rs:95-107 does: evals[d][node][copy], zero rows
    up to 2^bit_size"""
    per_copy = [gkr_ref.circuit_evaluate(circuit, inp, aux, r) for inp, aux in zip(inputs, witnesses)]
    evals = []
    for d, layer in enumerate(circuit.layers):
        rows = [[ev[d][i] for ev in per_copy] for i in range(layer.gates_count)]
        rows += [[0] * len(per_copy) for _ in range((1 << layer.bit_size) - layer.gates_count)]
        evals.append(rows)
    return evals


def eval_layer_batch(gates_raw, below_rows, r):
    """one layer over all copies: rows of the gates, then the zero rows"""
    n = len(below_rows[0])
    out = [[_op(op, below_rows[left][t], below_rows[right][t]) % r for t in range(n)] for op, left, right in gates_raw]
    return out + [[0] * n for _ in range((1 << gkr_ref._log2_ceil(len(out))) - len(out))]


def eval_outputs(out_rows, q, q_aside, r):
    """evaluate.rs:11-50 with the challenges given; out_rows[g][t]"""
    eq_q, eq_qa = eval_eq(q, r), eval_eq(q_aside, r)
    n = len(out_rows[0])
    eq_qs = [sum(out_rows[g][t] * eq_q[g] for g in range(len(out_rows))) % r for t in range(n)]       # :31-36
    return sum(a * b for a, b in zip(eq_qs, eq_qa)) % r                                               # :47


def weights(u, ql, qr, r):
    """xg_q, zk_sumcheck_proof.rs:84-88"""
    return [(a * u[0] + b * u[1]) % r for a, b in zip(eval_eq(ql, r), eval_eq(qr, r))]


# ------------------------------------------------------------------------------------------- the literal form
def sumcheck_literal(claim, u, q_vec, gates, circuit_evals, n, ng, next_round, r):
    """the table work of ZkSumcheckProof::prover, zk_sumcheck_proof.rs:56-442.  gates: (g, op, left, right); circuit_evals: ng rows
    of n.  Returns (polys, rs, r0, r1, (x, y))."""
    q_aside, ql, qr = q_vec
    log_ng, log_n = ng.bit_length() - 1, n.bit_length() - 1
    assert len(q_aside) == log_n and len(ql) == len(qr)                                    # :70-71
    polys = []
    eq_vec = eval_eq(q_aside, r)                                                           # :83
    xg_q = weights(u, ql, qr, r)
    temp_vec = [[e * xg % r for e in eq_vec] for xg in xg_q]                               # :89-95
    assert len(temp_vec) == len(gates)                                                     # :96
    circuit_evals = [list(row) for row in circuit_evals]
    rs, size = [], n
    for _ in range(log_n):                                                                 # sumcheck #1, :98-220
        size //= 2
        ev = {0: 0, 2: 0, 3: 0}
        for (_, op, left, right), tp in zip(gates, temp_vec):
            ev[0] += sum(tp[t] * _op(op, circuit_evals[left][t], circuit_evals[right][t]) for t in range(size))
            for k in (2, 3):
                tp_k, l_k, r_k = (combine_with_r(v, k, r) for v in (tp, circuit_evals[left], circuit_evals[right]))
                ev[k] += sum(tp_k[t] * _op(op, l_k[t], r_k[t]) for t in range(size))
        e0 = ev[0] % r
        coeffs = cubic_from_evals(e0, (claim - e0) % r, ev[2] % r, ev[3] % r, r)           # :157-177: [d, c, b, a]
        polys.append(coeffs)
        r_i = next_round(list(coeffs)) % r
        temp_vec = [combine_with_r(v, r_i, r) for v in temp_vec]                           # :191-196
        circuit_evals = [combine_with_r(v, r_i, r) for v in circuit_evals]                 # :198-203
        claim = poly_evaluate(coeffs, r_i, r)
        rs.append(r_i)
    v_vec = [row[0] for row in circuit_evals]                                              # :222-224
    temp_p_xg_vec = [v[0] for v in temp_vec]
    eq_node_vec = [eval_eq(convert_to_bit(i, log_ng), r) for i in range(ng)]               # :228-233
    left_eq_vec = [list(eq_node_vec[left]) for _, _, left, _ in gates]
    right_eq_vec = [list(eq_node_vec[right]) for _, _, _, right in gates]
    r0, size, v_left = [], ng, list(v_vec)
    for _ in range(log_ng):                                                                # sumcheck #2, :241-337
        size //= 2
        e0 = e2 = 0
        v_left_2 = combine_with_r(v_left, 2, r)
        for p, (_, op, _, right), left_eq in zip(temp_p_xg_vec, gates, left_eq_vec):
            e0 += sum(left_eq[i] * p * _op(op, v_left[i], v_vec[right]) for i in range(size))
            left_eq_2 = combine_with_r(left_eq, 2, r)
            e2 += sum(left_eq_2[i] * p * _op(op, v_left_2[i], v_vec[right]) for i in range(size))
        e0 %= r
        coeffs = quadratic_from_evals(e0, (claim - e0) % r, e2 % r, r)                     # :288-300: [c, b, a]
        polys.append(coeffs)
        r_i = next_round(list(coeffs)) % r
        left_eq_vec = [combine_with_r(v, r_i, r) for v in left_eq_vec]
        v_left = combine_with_r(v_left, r_i, r)
        claim = poly_evaluate(coeffs, r_i, r)
        r0.append(r_i)
    temp_p_xg_vec = [le[0] * p % r for le, p in zip(left_eq_vec, temp_p_xg_vec)]           # :339-344
    x = v_left[0]
    r1, size, v_right = [], ng, list(v_vec)
    for _ in range(log_ng):                                                                # sumcheck #3, :348-441 (its eval_1 sum is unused)
        size //= 2
        e0 = e2 = 0
        v_right_2 = combine_with_r(v_right, 2, r)
        for p, (_, op, _, _), right_eq in zip(temp_p_xg_vec, gates, right_eq_vec):
            e0 += sum(right_eq[i] * p * _op(op, x, v_right[i]) for i in range(size))
            right_eq_2 = combine_with_r(right_eq, 2, r)
            e2 += sum(right_eq_2[i] * p * _op(op, x, v_right_2[i]) for i in range(size))
        e0 %= r
        coeffs = quadratic_from_evals(e0, (claim - e0) % r, e2 % r, r)                     # :393-404
        polys.append(coeffs)
        r_i = next_round(list(coeffs)) % r
        right_eq_vec = [combine_with_r(v, r_i, r) for v in right_eq_vec]
        v_right = combine_with_r(v_right, r_i, r)
        claim = poly_evaluate(coeffs, r_i, r)
        r1.append(r_i)
    return polys, rs, r0, r1, (x, v_right[0])


# ------------------------------------------------------------------------------------------- the reduced form
def dp_round_evals(gates, rows, eq, w, length, r):
    """g(0), g(2), g(3) of one round of sum-check #1 over the live `length` of every table:
    g(X) = sum_{j < length/2} eq_X[j] sum_g w[g] op_g(L_X[j], R_X[j]), each table at lo + X (hi - lo)"""
    h = length // 2
    out = []
    for k in (0, 2, 3):
        at = lambda v, j: v[j] + k * (v[j + h] - v[j])             # noqa: E731
        out.append(sum(at(eq, j) * sum(w[g] * _op(op, at(rows[left], j), at(rows[right], j)) for g, op, left, right in gates)
                       for j in range(h)) % r)
    return tuple(out)


def dp_bind(table, length, x, r):
    """combine_with_r over the live `length`, in place as the device does it: [0, length/2) bound, the rest untouched"""
    h = length // 2
    return [(table[j] + x * (table[j + h] - table[j])) % r for j in range(h)] + list(table[h:])


def _libra_phase(phase, tables, fu, claim, next_round, r):
    tables = [list(t) for t in tables]
    polys, rs = [], []
    for _ in range(len(tables[0]).bit_length() - 1):
        e0, e2 = gkr_ref.round_evals(phase, tables, fu, r)
        coeffs = quadratic_from_evals(e0, (claim - e0) % r, e2, r)
        x = next_round(list(coeffs)) % r
        tables = [combine_with_r(t, x, r) for t in tables]
        claim = poly_evaluate(coeffs, x, r)
        polys.append(coeffs)
        rs.append(x)
    return polys, rs, tables[0][0], claim


def sumcheck_fast(claim, u, q_vec, gates, circuit_evals, n, ng, next_round, r):
    """the same proof from one eq table, one weight vector and Libra's bookkeeping tables"""
    q_aside, ql, qr = q_vec
    log_ng = ng.bit_length() - 1
    assert 1 << len(q_aside) == n and len(ql) == len(qr) and len(circuit_evals) == ng
    eq, w = eval_eq(q_aside, r), weights(u, ql, qr, r)
    assert len(w) == len(gates)
    rows = [list(row) for row in circuit_evals]
    polys, rs, length = [], [], n
    while length > 1:
        e0, e2, e3 = dp_round_evals(gates, rows, eq, w, length, r)
        coeffs = cubic_from_evals(e0, (claim - e0) % r, e2, e3, r)
        x = next_round(list(coeffs)) % r
        rows, eq = [dp_bind(t, length, x, r) for t in rows], dp_bind(eq, length, x, r)
        length //= 2
        claim = poly_evaluate(coeffs, x, r)
        polys.append(coeffs)
        rs.append(x)
    v = [row[0] for row in rows]
    p = [wg * eq[0] % r for wg in w]
    polys_2, r0, x, claim = _libra_phase(1, [v, *gkr_ref.eval_hg(p, v, gates, log_ng, r)], None, claim, next_round, r)
    mul, add = gkr_ref.eval_fgu(p, eval_eq(r0, r), gates, log_ng, r)
    polys_3, r1, y, claim = _libra_phase(2, [v, mul, add], x, claim, next_round, r)
    return polys + polys_2 + polys_3, rs, r0, r1, (x, y)


# ------------------------------------------------------------------------------------------- the layer loop
def prove_layers(circuit, evals, n, q_aside, q, result_u, next_round, next_u, r, sumcheck=sumcheck_literal):
    """the loop of HyraxProof::prover, hyrax_proof.rs:72-147: (proofs, q', ql, qr), proofs[i] = (polys, (rs, r0, r1), (x, y))"""
    u = (1, 0)
    q_aside, ql = [t % r for t in q_aside], [t % r for t in q]
    qr = list(ql)
    claim = result_u % r
    proofs = []
    for d in range(circuit.depth - 1, 0, -1):
        ng = 1 << circuit.layers[d - 1].bit_size                                           # :93-94
        polys, rs, r0, r1, (x, y) = sumcheck(claim, u, (q_aside, ql, qr), circuit.layers[d].gates, evals[d - 1], n, ng, next_round, r)
        proofs.append((polys, (rs, r0, r1), (x, y)))
        q_aside, ql, qr = rs, r0, r1                                                       # :125-127
        if d > 1:                                                                          # :134-145
            u = tuple(v % r for v in next_u())
            claim = (x * u[0] + y * u[1]) % r
    return proofs, q_aside, ql, qr


def prover(circuit, inputs, witnesses, q_aside, q, next_round, next_u, r, sumcheck=sumcheck_literal):
    """HyraxProof::prover without commitments: (proofs, evals, result_u, (q', ql, qr))"""
    evals = circuit_evaluate_batch(circuit, inputs, witnesses, r)
    result_u = eval_outputs(evals[-1], q, q_aside, r)                                      # :72
    proofs, qa, ql, qr = prove_layers(circuit, evals, len(inputs), q_aside, q, result_u, next_round, next_u, r, sumcheck)
    return proofs, evals, result_u, (qa, ql, qr)


def eval_witness(witnesses, q_aside, ql, qr, r):
    """eval_value(witness_vec, q' || ql[1:]) and (..., q' || qr[1:]), hyrax_proof.rs:56-62, 149-178"""
    wl = 1 << gkr_ref._log2_ceil(max(len(witnesses[0]), 1))
    vec = [v for w in witnesses for v in list(w) + [0] * (wl - len(w))]
    return tuple(gkr_ref.eval_value(vec, list(q_aside) + list(tail[1:]), r) for tail in (ql, qr))


def verify(circuit, proofs, out_rows, input_rows, q_aside, q, next_round, next_u, r):
    """A plain, commitment-free verifier (the reference checks the same relations under commitments, construct_matrix,
    evaluate.rs:151-235): p(0) + p(1) = claim per round, the final claim
    eq(q', rs) sum_g w[g] eq(r0)[left_g] eq(r1)[right_g] op_g(x, y), and at the bottom x and y against the input layer."""
    n = len(out_rows[0])
    log_n = n.bit_length() - 1
    u = (1, 0)
    q_aside, ql = [t % r for t in q_aside], [t % r for t in q]
    qr = list(ql)
    claim = eval_outputs(out_rows, q, q_aside, r)
    if len(proofs) != circuit.depth - 1:
        return False
    x = y = 0
    rs, r0, r1 = q_aside, ql, qr
    for i, (polys, _, (x, y)) in enumerate(proofs):
        d = circuit.depth - 1 - i
        log_ng = circuit.layers[d - 1].bit_size
        if len(polys) != log_n + 2 * log_ng:
            return False
        chal = []
        for k, poly in enumerate(polys):
            if len(poly) != (4 if k < log_n else 3):
                return False
            if (poly_evaluate(poly, 0, r) + poly_evaluate(poly, 1, r)) % r != claim:
                return False
            t = next_round(list(poly)) % r
            chal.append(t)
            claim = poly_evaluate(poly, t, r)
        rs, r0, r1 = chal[:log_n], chal[log_n:log_n + log_ng], chal[log_n + log_ng:]
        w = weights(u, ql, qr, r)
        eq_r0, eq_r1 = eval_eq(r0, r), eval_eq(r1, r)
        wiring = sum(w[g] * eq_r0[left] * eq_r1[right] * _op(op, x, y) for g, op, left, right in circuit.layers[d].gates)
        if claim != eval_eq_x_y(q_aside, rs, r) * wiring % r:
            return False
        q_aside, ql, qr = rs, r0, r1
        if d > 1:
            u = tuple(v % r for v in next_u())
            claim = (x * u[0] + y * u[1]) % r
    eq_rs = eval_eq(rs, r)
    at = lambda point: sum(e * sum(a * b for a, b in zip(row, eq_rs)) for e, row in zip(eval_eq(point, r), input_rows)) % r   # noqa: E731
    return x % r == at(r0) and y % r == at(r1)
