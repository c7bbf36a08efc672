"""Python-integer restatement of the SPARK memory-checking layer of the Spartan prover and of the product-circuit evaluation
proof, against the line numbers of spartan/src/spark.rs, prover.rs and verify.rs.  Field elements are canonical integers mod r;
no product imports.  Commitments and the merlin transcript are left out; three callbacks stand where the reference draws from it:
    next_coeffs(count)                      -> `count` integers            ("rand_coeffs_next_layer")
    next_round(coeffs)                      -> the sum-check challenge     ("challenge_nextround")
    next_layer(left, right, dotp or None)   -> r_layer                     ("challenge_r_layer")
The prover and the verifier call them in the same order with the same arguments.
Only power-of-two lengths: the reference's padding of an odd layer with 1 (spark.rs:325-328) is never reached by them."""
from tests.sumcheck_ref import cubic_batched, eval_eq, evaluate


def memory_in_the_head(addrs_list, m):
    """spark.rs:132-176 -> (read_ts_list, audit_ts) as integers"""
    audit_ts = [0] * m
    read_ts_list = []
    for addrs in addrs_list:
        read_ts = [0] * len(addrs)
        for i, addr in enumerate(addrs):                                                   # :144-150
            r_ts = audit_ts[addr]
            read_ts[i] = r_ts
            audit_ts[addr] = r_ts + 1
        read_ts_list.append(read_ts)
    return read_ts_list, audit_ts


def circuit_hash(a_list, v_list, t_list, gamma, r):
    """spark.rs:298-312"""
    assert len(a_list) == len(v_list) == len(t_list)
    return [(a * gamma * gamma + v * gamma + t) % r for a, v, t in zip(a_list, v_list, t_list)]


def construct_product_circuit(values, r):
    """spark.rs:315-347 -> (left_vec, right_vec)"""
    lst = [v % r for v in values]
    assert len(lst) >= 2 and len(lst) & (len(lst) - 1) == 0
    left_vec, right_vec = [], []
    for _ in range(len(lst).bit_length() - 1):
        tlen = len(lst) // 2
        left, right = lst[:tlen], lst[tlen:]
        lst = [x * y % r for x, y in zip(left, right)]
        left_vec.append(left)
        right_vec.append(right)
    return left_vec, right_vec


def evaluate_product_circuit(circuit, r):
    """spark.rs:349-359"""
    left_vec, right_vec = circuit
    assert len(left_vec[-1]) == 1 and len(right_vec[-1]) == 1
    return left_vec[-1][0] * right_vec[-1][0] % r


def layer_offset(n, l):
    """element at which layer l (n >> l elements) starts in the flat buffer of 2n - 2 elements"""
    return 2 * n - ((2 * n) >> l)


def flatten(circuit):
    """every layer of a circuit, layer l = left_vec[l] + right_vec[l], one after another: 2n - 2 elements"""
    return [v for left, right in zip(*circuit) for v in left + right]


def evaluate_dot_product_circuit(row, col, val, r):
    """spark.rs:361-372"""
    return sum(x * y * z for x, y, z in zip(row, col, val)) % r


def memory_checking(lists, mem, read_ts_list, audit_ts, e_list, gamma, r):
    """spark.rs:209-296 -> dict(init, read, write, audit) of circuits; the product check of :285 raises AssertionError"""
    gamma1, gamma2 = gamma
    assert len(lists) == len(read_ts_list) == len(e_list) and len(mem) == len(audit_ts)
    init_a = list(range(len(mem)))                                                         # :224-226
    sub = lambda h: [(x - gamma2) % r for x in h]                                          # noqa: E731   :250-273
    init_prod = construct_product_circuit(sub(circuit_hash(init_a, mem, [0] * len(mem), gamma1, r)), r)
    read_prod, write_prod = [], []
    for lst, read_ts, e in zip(lists, read_ts_list, e_list):                               # :232-241
        write_ts = [t + 1 for t in read_ts]
        read_prod.append(construct_product_circuit(sub(circuit_hash(lst, e, read_ts, gamma1, r)), r))
        write_prod.append(construct_product_circuit(sub(circuit_hash(lst, e, write_ts, gamma1, r)), r))
    audit_prod = construct_product_circuit(sub(circuit_hash(init_a, mem, audit_ts, gamma1, r)), r)
    init = evaluate_product_circuit(init_prod, r)                                          # :276-285
    read = write = 1
    for c in read_prod:
        read = read * evaluate_product_circuit(c, r) % r
    for c in write_prod:
        write = write * evaluate_product_circuit(c, r) % r
    audit = evaluate_product_circuit(audit_prod, r)
    assert init * write % r == read * audit % r, "memory check: init * write != read * audit"
    return dict(init=init_prod, read=read_prod, write=write_prod, audit=audit_prod)


def product_circuit_eval_prover(circuits, dotp, next_coeffs, next_round, next_layer, r):
    """prover.rs:1313-1440.  circuits: (left_vec, right_vec) each, all of one size; dotp: (row, col, val) triples as long as a half
    of layer 0.  Returns (layers, claim_dotp, rands): layers = [(polys, claim_prod_left, claim_prod_right)] from the top layer down,
    claim_dotp = (rows, cols, vals) finals.  Works on copies."""
    assert circuits
    layer_num = len(circuits[0][0])
    claims = [evaluate_product_circuit(c, r) for c in circuits]                            # :1323-1325
    layers, rands = [], []
    final_dotp = ([], [], [])
    for i in reversed(range(layer_num)):                                                   # :1331
        lefts = [c[0][i] for c in circuits]
        rights = [c[1][i] for c in circuits]
        rand_par = eval_eq(rands, r)                                                       # :1348
        assert len(rand_par) == len(lefts[0])
        rows, cols, vals = [], [], []
        with_dotp = i == 0 and len(dotp) > 0
        if with_dotp:                                                                      # :1353-1365
            for row, col, val in dotp:
                assert len(row) == len(col) == len(val) == len(rand_par)
                rows.append(row)
                cols.append(col)
                vals.append(val)
                claims.append(evaluate_dot_product_circuit(row, col, val, r))
        coeffs = [c % r for c in next_coeffs(len(claims))]                                 # :1367-1373
        claim = sum(x * w for x, w in zip(claims, coeffs)) % r                             # :1375-1377
        polys, rand_prod, claim_prod, claim_dotp = cubic_batched(lefts, rights, rand_par, rows, cols, vals, coeffs, claim,
                                                                 next_round, r)            # :1380-1392
        left, right, _ = claim_prod
        if with_dotp:
            final_dotp = claim_dotp                                                        # :1403-1404
        r_layer = next_layer(list(left), list(right), tuple(list(t) for t in claim_dotp) if with_dotp else None) % r
        claims = [(x + r_layer * (y - x)) % r for x, y in zip(left, right)]                # :1420-1422
        rands = [r_layer] + list(rand_prod)                                                # :1424-1425
        layers.append((polys, list(left), list(right)))
    return layers, tuple(list(t) for t in final_dotp), rands


def sum_check_cubic_verify(polys, num_rounds, claim, next_round, r):
    """verify.rs:817-841"""
    assert len(polys) == num_rounds
    rs = []
    for poly in polys:
        assert (evaluate(poly, 0, r) + evaluate(poly, 1, r)) % r == claim % r, "sum-check: g(0) + g(1) != claim"
        x = next_round(list(poly)) % r
        claim = evaluate(poly, x, r)
        rs.append(x)
    return rs, claim


def product_circuit_eval_verify(proof, claims_prod_circuit, claims_dotp_circuit, n, next_coeffs, next_round, next_layer, r):
    """verify.rs:717-815; proof = (layers, claim_dotp) as the prover returns them.  Raises AssertionError on a false proof.
    Returns (claims_to_verify, claims_to_verify_dotp, rands)."""
    layers, proof_dotp = proof
    layer_num = n.bit_length() - 1
    claims = [c % r for c in claims_prod_circuit]
    assert len(layers) == layer_num
    num_rounds, rands, claims_dotp = 0, [], []
    for i in range(layer_num):
        last = i == layer_num - 1
        if last:
            claims = claims + [c % r for c in claims_dotp_circuit]                         # :733-735
        coeffs = [c % r for c in next_coeffs(len(claims))]
        claim = sum(x * w for x, w in zip(claims, coeffs)) % r
        polys, left, right = layers[i]
        rs, claim_final = sum_check_cubic_verify(polys, num_rounds, claim, next_round, r)  # :749-754
        assert len(left) == len(right) == len(claims_prod_circuit)
        assert len(rands) == len(rs)
        eq = 1
        for x, y in zip(rs, rands):                                                        # :765-767
            eq = eq * (x * y + (1 - x) * (1 - y)) % r
        expected = sum(w * (x * y % r * eq) for w, x, y in zip(coeffs, left, right)) % r   # :769-771
        rows, cols, vals = proof_dotp
        with_dotp = last and len(rows) > 0
        if last:                                                                           # :773-785
            for k in range(len(rows)):
                expected = (expected + coeffs[len(left) + k] * rows[k] * cols[k] * vals[k]) % r
        assert expected == claim_final, "layer %d: the final claim does not match the evaluations" % i
        r_layer = next_layer(list(left), list(right), tuple(list(t) for t in proof_dotp) if with_dotp else None) % r
        claims = [(x + r_layer * (y - x)) % r for x, y in zip(left, right)]                # :792-794
        if last:                                                                           # :795-808
            for k in range(len(rows) // 2):
                for t in (rows, cols, vals):
                    claims_dotp.append((t[2 * k] + r_layer * (t[2 * k + 1] - t[2 * k])) % r)
        num_rounds += 1
        rands = [r_layer] + rs
    return claims, claims_dotp, rands
