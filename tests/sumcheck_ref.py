"""Python-integer restatement of the sum-check code of the Spartan prover, against the line numbers of spartan/src/polynomial.rs
and spartan/src/prover.rs.  Field elements are canonical integers mod r; no product imports.  Commitments, blinds and the merlin
transcript are left out: `next_challenge(coeffs)` stands where the reference draws `challenge_nextround`."""


def eval_eq(rx, r):
    """polynomial.rs:8-24"""
    evals = [1] * (1 << len(rx))
    size = 1
    for i in range(len(rx)):
        scalar = rx[len(rx) - i - 1]
        for j in range(size):
            evals[size + j] = scalar * evals[j] % r
            evals[j] = (1 - scalar) * evals[j] % r
        size *= 2
    return evals


def eval_eq_x_y(rx, ry, r):
    """polynomial.rs:26-32"""
    assert len(rx) == len(ry)
    out = 1
    for x, y in zip(rx, ry):
        out = out * ((1 - x) * (1 - y) + x * y) % r
    return out


def combine_with_n(values, t, r):
    """polynomial.rs:121-129"""
    n = len(values) // 2
    return [(t * values[i + n] + (1 - t) * values[i]) % r for i in range(n)]


def combine_with_r(values, x, r):
    """polynomial.rs:131-138; returns the truncated vector"""
    return combine_with_n(values, x, r)


def evaluate(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def cubic_from_evals(e0, e1, e2, e3, r):
    """prover.rs:499-516: [d, c, b, a]"""
    a = (-e0 + 2 * e1 + e1 - 2 * e2 - e2 + e3) * pow(6, -1, r) % r
    b = (2 * e0 - 4 * e1 - e1 + 4 * e2 - e3) * pow(2, -1, r) % r
    c = (e1 - e0 - a - b) % r
    return [e0 % r, c, b, a]


def quadratic_from_evals(e0, e1, e2, r):
    """prover.rs:646-655: [c, b, a]"""
    a = (e0 - 2 * e1 + e2) * pow(2, -1, r) % r
    return [e0 % r, (e1 - a - e0) % r, a]


def _g1(eq, a, b, c, r):
    return sum(e * (x * y - z) for e, x, y, z in zip(eq, a, b, c)) % r


EQ_AB_MINUS_C, PROD2, PROD3 = 0, 1, 2
ARITY = {EQ_AB_MINUS_C: 4, PROD2: 2, PROD3: 3}
POINTS = {EQ_AB_MINUS_C: (0, 2, 3), PROD2: (0, 2), PROD3: (0, 2, 3)}


def round_evals(kind, tables, r):
    """The evaluations one round takes of one term: sum_j g(combine_with_n(table, t)[j]) for t in POINTS[kind], tables in the
    order eq, a, b, c / a, b / a, b, c.  combine_with_n(v, t)[j] = lo + t (hi - lo) is left unreduced until the sum (same value
    mod r), which keeps a 2^16-entry term affordable."""
    n = len(tables[0]) // 2
    out = []
    for t in POINTS[kind]:
        vals = [[lo + t * (hi - lo) for lo, hi in zip(tb[:n], tb[n:])] for tb in tables]
        if kind == EQ_AB_MINUS_C:
            out.append(sum(e * (a * b - c) for e, a, b, c in zip(*vals)) % r)
        elif kind == PROD2:
            out.append(sum(a * b for a, b in zip(*vals)) % r)
        else:
            out.append(sum(a * b * c for a, b, c in zip(*vals)) % r)
    return tuple(out)


def phase_one(eq, a, b, c, claim, next_challenge, r):
    """sum_check_proof_phase_one, prover.rs:473-591.  Returns (polys, rx, (va, vb, vc, veq))."""
    eq, a, b, c = list(eq), list(a), list(b), list(c)
    assert len(a) == len(b) == len(c) == len(eq)
    polys, rx = [], []
    for _ in range(len(eq).bit_length() - 1):
        size = len(eq) // 2
        e0 = _g1(eq[:size], a, b, c, r)                                                    # :476-478
        e1 = (claim - e0) % r                                                              # :480
        e2 = _g1(*(combine_with_n(t, 2, r) for t in (eq, a, b, c)), r)                     # :483-489
        e3 = _g1(*(combine_with_n(t, 3, r) for t in (eq, a, b, c)), r)                     # :491-497
        poly = cubic_from_evals(e0, e1, e2, e3, r)
        x = next_challenge(list(poly)) % r                                                 # :528-530
        a, b, c, eq = (combine_with_r(t, x, r) for t in (a, b, c, eq))                     # :531-534
        claim = evaluate(poly, x, r)                                                       # :538, :577
        polys.append(poly)
        rx.append(x)
    return polys, rx, (a[0], b[0], c[0], eq[0])


def phase_two(abc, z, claim, next_challenge, r):
    """sum_check_proof_phase_two, prover.rs:632-722.  Returns (polys, ry, (vs, vz))."""
    abc, z = list(abc), list(z)
    assert len(abc) == len(z)
    polys, ry = [], []
    size = len(z)
    for _ in range(len(z).bit_length() - 1):
        size //= 2
        e0 = sum(z[j] * abc[j] for j in range(size)) % r                                   # :637
        e1 = (claim - e0) % r
        e2 = sum(x * y for x, y in zip(combine_with_n(abc, 2, r), combine_with_n(z, 2, r))) % r   # :642-644
        poly = quadratic_from_evals(e0, e1, e2, r)
        x = next_challenge(list(poly)) % r
        claim = evaluate(poly, x, r)                                                       # :670, :710
        abc, z = combine_with_r(abc, x, r), combine_with_r(z, x, r)                        # :682-683
        polys.append(poly)
        ry.append(x)
    return polys, ry, (abc[0], z[0])


def _cubic_term(a, b, c, r):
    """prover.rs:1479-1496: the doublings spelled out as the reference does"""
    n = len(a) // 2
    e0 = e2 = e3 = 0
    for i in range(n):
        e0 += a[i] * b[i] * c[i]
        e2 += (2 * a[n + i] - a[i]) * (2 * b[n + i] - b[i]) * (2 * c[n + i] - c[i])
        e3 += (2 * a[n + i] + a[n + i] - 2 * a[i]) * (2 * b[n + i] + b[n + i] - 2 * b[i]) * (2 * c[n + i] + c[n + i] - 2 * c[i])
    return e0 % r, e2 % r, e3 % r


def cubic_batched(a_par, b_par, c_par, a_seq, b_seq, c_seq, coeffs, claim, next_challenge, r):
    """sum_check_cubic_prover, prover.rs:1467-1606.  Returns (polys, r, (a_par, b_par, c_par), (a_seq, b_seq, c_seq)) finals."""
    a_par, b_par, c_par = [list(t) for t in a_par], [list(t) for t in b_par], list(c_par)
    a_seq, b_seq, c_seq = [list(t) for t in a_seq], [list(t) for t in b_seq], [list(t) for t in c_seq]
    polys, rs = [], []
    rounds = (len(c_par) if a_par else len(a_seq[0])).bit_length() - 1
    for _ in range(rounds):
        evals = [_cubic_term(a, b, c_par, r) for a, b in zip(a_par, b_par)]
        evals += [_cubic_term(a, b, c, r) for a, b, c in zip(a_seq, b_seq, c_seq)]
        assert len(coeffs) == len(evals)
        s0 = sum(e[0] * w for e, w in zip(evals, coeffs)) % r                             # :1531-1534
        s1 = (claim - s0) % r
        s2 = sum(e[1] * w for e, w in zip(evals, coeffs)) % r
        s3 = sum(e[2] * w for e, w in zip(evals, coeffs)) % r
        poly = cubic_from_evals(s0, s1, s2, s3, r)
        x = next_challenge(list(poly)) % r
        c_par = combine_with_r(c_par, x, r)                                                # :1560-1580
        a_par = [combine_with_r(t, x, r) for t in a_par]
        b_par = [combine_with_r(t, x, r) for t in b_par]
        a_seq = [combine_with_r(t, x, r) for t in a_seq]
        b_seq = [combine_with_r(t, x, r) for t in b_seq]
        c_seq = [combine_with_r(t, x, r) for t in c_seq]
        claim = evaluate(poly, x, r)
        polys.append(poly)
        rs.append(x)
    return (polys, rs, ([t[0] for t in a_par], [t[0] for t in b_par], c_par[0]),
            ([t[0] for t in a_seq], [t[0] for t in b_seq], [t[0] for t in c_seq]))


def matrix_vec(m, z, r):
    """evaluate_matrix_vec, polynomial.rs:84-100; m: rows of (value, column) with the column already mapped into z"""
    return [sum(v * z[col] for v, col in row) % r for row in m]


def matrix_vec_col(m, coeffs, num_cols, r):
    """evaluate_matrix_vec_col, polynomial.rs:102-119"""
    ms = [0] * num_cols
    for row, entries in enumerate(m):
        for v, col in entries:
            ms[col] = (ms[col] + v * coeffs[row]) % r
    return ms


def r1cs_backbone(ma, mb, mc, z, tau, challenge_1, abc_challenges, challenge_2, r):
    """r1cs_satisfied_prover, prover.rs:265-371, without commitments.  abc_challenges: (va, vb, vc, veq) -> (r_a, r_b, r_c).
    Returns (polys_1, rx, (va, vb, vc, veq), polys_2, ry, (vs, vz))."""
    eq_tau = eval_eq(tau, r)                                                               # :265
    az, bz, cz = matrix_vec(ma, z, r), matrix_vec(mb, z, r), matrix_vec(mc, z, r)         # :266-268
    polys_1, rx, vals = phase_one(eq_tau, az, bz, cz, 0, challenge_1, r)                   # :270-281
    va, vb, vc, _ = vals
    r_a, r_b, r_c = abc_challenges(*vals)
    claim_2 = (va * r_a + vb * r_b + vc * r_c) % r                                         # :348
    evals_rx = eval_eq(rx, r)                                                              # :351
    ea, eb, ec = (matrix_vec_col(m, evals_rx, len(z), r) for m in (ma, mb, mc))            # :352-354
    evals = [(r_a * x + r_b * y + r_c * w) % r for x, y, w in zip(ea, eb, ec)]             # :357-359
    polys_2, ry, vals_2 = phase_two(evals, z, claim_2, challenge_2, r)                     # :361-371
    return polys_1, rx, vals, polys_2, ry, vals_2
