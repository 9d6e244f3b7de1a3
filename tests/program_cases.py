"""Quotient programs of a CHOSEN shape (beside quotient_cases.py, whose programs are random): how many intermediates the compiled program keeps live — which
decides the launch shape of the interpreter and what the generated kernels carry across their cuts — and graph forms halo2's Evaluator never
emits but the ZKQ1 blob reader accepts.  Every builder returns an evaluation.Program; what the compiler makes of it (slots, split, rotations) is asserted by the
caller through the Backend, never assumed here."""
import re

from zk_dcap_verifier_amd import evaluation as ev

PERM_POOL = [(0, 0), (0, 1), (1, 0), (0, 3)]          # (0 advice | 1 fixed, index): one full set of three columns and a second set of one at cs_degree 5
N_FIXED, N_ADVICE = 1, 4


def _lookup_graph():
    """(Horner(a0, [a1], theta) + beta) * (f0 + gamma): halo2's compressed input times compressed table"""
    g = ev.Graph()
    r0 = g.add_rotation(0)
    ci = g.add_calculation(ev.HORNER, ev.vs(ev.ADVICE, 0, r0), [ev.vs(ev.ADVICE, 1, r0)], ev.vs(ev.THETA))
    a = g.add_calculation(ev.ADD, ci, ev.vs(ev.BETA))
    b = g.add_calculation(ev.ADD, ev.vs(ev.FIXED, 0, r0), ev.vs(ev.GAMMA))
    g.add_calculation(ev.MUL, a, b)
    return g


def _program(k, custom, perm=0, lookups=0, cs_degree=5, n_challenges=0, lookup_graphs=None):
    lg = list(lookup_graphs) if lookup_graphs is not None else [_lookup_graph() for _ in range(lookups)]
    return ev.Program(k=k, extended_k=k + 2, n_fixed=N_FIXED, n_advice=N_ADVICE, n_instance=0, n_challenges=n_challenges, blinding_factors=5, cs_degree=cs_degree,
                      perm_columns=PERM_POOL[:perm], custom_gates=custom, lookups=lg)


def _close(g, gates):
    """halo2's Evaluator::new ends the custom-gate graph with Horner(PreviousValue, gate polynomials, Y)"""
    g.add_calculation(ev.HORNER, ev.vs(ev.PREVIOUS), list(gates), ev.vs(ev.Y))
    return g


def _horner_value(g, i):
    """a degree-3 value over three columns and three rotations; a Horner is never rematerialised, so it holds its slot from its first to its last reader"""
    r0 = g.add_rotation(0)
    return g.add_calculation(ev.HORNER, ev.vs(ev.ADVICE, i % 4, r0),
                             [ev.vs(ev.FIXED, 0, g.add_rotation(i % 7 - 3)), ev.vs(ev.ADVICE, (i + 1) % 4, r0)],
                             ev.vs(ev.ADVICE, (i + 2) % 4, g.add_rotation(i % 5 - 2)))


def live_program(L, k, perm=0, lookups=0, cs_degree=5):
    """L values that are all read twice, first by a sum and then, in the same order, by a product: each stays live across the whole sum, so the compiled program
    needs L slots for them and one for the running value"""
    g = ev.Graph()
    v = [_horner_value(g, i) for i in range(L)]
    s = v[0]
    for i in range(1, L):
        s = g.add_calculation(ev.ADD, s, v[i])
    for i in range(L):
        s = g.add_calculation(ev.MUL, s, v[i])
    small = g.add_calculation(ev.MUL, ev.vs(ev.FIXED, 0, g.add_rotation(0)), ev.vs(ev.ADVICE, 1, g.add_rotation(0)))
    return _program(k, _close(g, [s, small]), perm, lookups, cs_degree)


# slots the compiler must report -> live_program arguments (L, perm, lookups).  9, 34 and 81 carry a two-set permutation and lookups, so that the degree parts
# run at high slot counts as well
LADDER = {5: (4, 0, 0), 6: (5, 0, 0), 9: (8, 4, 1), 10: (9, 0, 0), 33: (32, 0, 0), 34: (33, 4, 1), 81: (80, 4, 2)}
MAX_SLOTS = 81                                           # 80 LDS slots x 64 threads x 32 bytes = 160 KiB, the LDS of a CU


def ladder_program(slots, k):
    L, perm, lookups = LADDER[slots]
    return live_program(L, k, perm, lookups)


def launch_shape(slots, rows, threads):
    """quotient_run's choice for a program of `slots` slots on `rows` rows under tune quot_threads = `threads`: (T, dynamic LDS bytes).  A restatement of
    quot_launch_shape (csrc/quotient.hip), so that a test can say which rung it stands on without a library at hand;
    test_structured_programs.test_launch_shape_of_every_rung pins it against that function.  Slot 0 is a register"""
    T = min(threads, 256, rows)
    while T > 64 and (slots - 1) * T * 32 > 32 * 1024:
        T >>= 1
    return T, (slots - 1) * T * 32


def part_slots(be, lib_source, handle):
    """slots of the whole program and of its high and low parts, read from the generated source of each (every slot a micro-op writes appears as `sN = t;`): the C ABI
    reports the whole program's count only.  A part whose source writes no slot at all counts as 1, the compiler's own floor (QuotProgram::n_slots of a program that
    keeps everything in the accumulator): 1 means "no slot beyond the accumulator", not one slot in use.  lib_source: test_quotient_jit._source (emulator build)"""
    out = []
    for part in (0, 1, 2):
        src, _, _ = lib_source(be, handle, part, 200)
        written = [int(m) for m in re.findall(r"; s(\d+) = t; \}", src)]
        out.append(max(written) + 1 if written else 1)
    return tuple(out)


# ---- forms the random builder never produces -------------------------------------------------------------------------------------------------------------------------

def _gate(g, i=0):
    """f0 * (a_i * a_(i+1)(wX) - a_(i+2)): degree 3"""
    r0, r1 = g.add_rotation(0), g.add_rotation(1)
    m = g.add_calculation(ev.MUL, ev.vs(ev.ADVICE, i % 4, r0), ev.vs(ev.ADVICE, (i + 1) % 4, r1))
    s = g.add_calculation(ev.SUB, m, ev.vs(ev.ADVICE, (i + 2) % 4, r0))
    return g.add_calculation(ev.MUL, ev.vs(ev.FIXED, 0, r0), s)


def form_single_identity(orc, k):
    """the custom-gate graph ends in a plain value, not in Horner(PreviousValue, .., Y): ONE identity of the high part"""
    g = ev.Graph()
    a, b = _gate(g, 0), _gate(g, 1)
    g.add_calculation(ev.MUL, a, b)
    return _program(k, g, perm=4, lookups=2)


def form_empty_gates(orc, k):
    return _program(k, ev.Graph(), perm=4, lookups=2)


def form_horner_without_parts(orc, k):
    """Horner(PreviousValue, [], Y) is PreviousValue, that is zero; the gate computed before it has no reader"""
    g = ev.Graph()
    _gate(g, 0)
    return _program(k, _close(g, []), perm=4, lookups=1)


def form_bare_parts(orc, k):
    """gate polynomials that are a bare column, a bare constant and a challenge (degrees 1, 0, 0: folds of memory operands, all in the low part) between two real gates"""
    g = ev.Graph()
    c = g.add_constant(orc.fr_from_ints([0x1234567890ABCDEF1122334455667788])[0])
    a, b = _gate(g, 0), _gate(g, 2)
    return _program(k, _close(g, [a, ev.vs(ev.ADVICE, 2, g.add_rotation(-1)), c, ev.vs(ev.CHALLENGE, 0), b]), perm=4, lookups=1, n_challenges=1)


def form_zero_start_horner(orc, k):
    """Horner(0, [column], theta) and Horner(0, [column, value], theta) — the zero start whose first part is a memory operand — as gate factors and as the WHOLE of a
    lookup's table expression"""
    def chains(g):
        zero = g.add_constant(orc.fr_from_ints([0])[0])
        r0, r1 = g.add_rotation(0), g.add_rotation(1)
        h1 = g.add_calculation(ev.HORNER, zero, [ev.vs(ev.ADVICE, 0, r1)], ev.vs(ev.THETA))
        v = g.add_calculation(ev.MUL, ev.vs(ev.ADVICE, 2, r0), ev.vs(ev.ADVICE, 3, r1))
        h2 = g.add_calculation(ev.HORNER, zero, [ev.vs(ev.ADVICE, 1, r0), v], ev.vs(ev.THETA))
        return h1, h2
    g = ev.Graph()
    h1, h2 = chains(g)
    f0 = ev.vs(ev.FIXED, 0, g.add_rotation(0))
    g1, g2 = g.add_calculation(ev.MUL, h1, f0), g.add_calculation(ev.MUL, h2, f0)
    one_part, two_parts = ev.Graph(), ev.Graph()
    zero = one_part.add_constant(orc.fr_from_ints([0])[0])
    one_part.add_calculation(ev.HORNER, zero, [ev.vs(ev.FIXED, 0, one_part.add_rotation(-1))], ev.vs(ev.THETA))
    chains(two_parts)                                                  # (its last calculation, the two-part chain, is the graph's result; the one-part chain has no reader)
    return _program(k, _close(g, [g1, g2]), perm=4, lookup_graphs=[one_part, two_parts, _lookup_graph()])


def form_same_value_twice(orc, k):
    """op(v, v) with v a Horner result that nothing else reads: both operands die in the same instruction and their slot is handed back once"""
    g = ev.Graph()
    gates = []
    for i, op in enumerate((ev.MUL, ev.SUB, ev.ADD)):
        v = _horner_value(g, i)
        gates.append(g.add_calculation(op, v, v))
    v = _horner_value(g, 3)
    gates.append(g.add_calculation(ev.HORNER, v, [v], v))
    return _program(k, _close(g, gates), perm=4, lookups=1)


def form_difference_of_a_value_with_itself(orc, k):
    """the whole numerator is SUB(v, v): every row must come out as the canonical zero (slots hold values in [0, 2p]; 2p - 2p, p - p and 0 are all zero mod p)"""
    g = ev.Graph()
    v = _horner_value(g, 1)
    g.add_calculation(ev.SUB, v, v)
    return _program(k, g)


def form_written_twice(orc, k):
    """intermediate 0 is written twice and read between and after the writes.  halo2 never emits this (add_calculation gives every calculation a fresh target); the
    oracle's definition is the one of a memory cell — a reader sees the last write before it — and that is what is pinned here"""
    g = ev.Graph()
    r0, r1 = g.add_rotation(0), g.add_rotation(1)
    i0, i1, i2, i3 = (ev.vs(ev.INTERMEDIATE, t) for t in range(4))
    g.calculations += [(ev.MUL, 0, (ev.vs(ev.ADVICE, 0, r0), ev.vs(ev.ADVICE, 1, r1))),
                       (ev.ADD, 1, (i0, ev.vs(ev.FIXED, 0, r0))),             # reads the first write
                       (ev.SUB, 0, (i1, ev.vs(ev.ADVICE, 2, r1))),            # second write, from a value that depends on the first
                       (ev.MUL, 2, (i0, i1)),                                 # reads the second write
                       (ev.HORNER, 3, (ev.vs(ev.PREVIOUS), [i2, i0, i1], ev.vs(ev.Y)))]
    g.num_intermediates = 4
    return _program(k, g, perm=4, lookups=1)


def form_rotations_beyond_the_domain(orc, k=2):
    """rotations 5, -7, 4, -4 on a domain of 2^2 rows: the whole-domain run scales them by 2^(extended_k - k), the coset run does not, both take them modulo their size
    (4 and -4 are then the rotation 0 on a coset and on the domain alike, 5 is 1 and -7 is 1)"""
    assert k == 2
    g = ev.Graph()
    rots = [g.add_rotation(r) for r in (5, -7, 4, -4)]
    m = g.add_calculation(ev.MUL, ev.vs(ev.ADVICE, 0, rots[0]), ev.vs(ev.ADVICE, 1, rots[1]))
    s = g.add_calculation(ev.SUB, m, ev.vs(ev.ADVICE, 2, rots[2]))
    a = g.add_calculation(ev.MUL, ev.vs(ev.FIXED, 0, rots[3]), s)
    lg = _lookup_graph()
    lr = [lg.add_rotation(r) for r in (-7, 4)]
    t = lg.add_calculation(ev.MUL, ev.vs(ev.INTERMEDIATE, lg.num_intermediates - 1), ev.vs(ev.ADVICE, 3, lr[0]))
    lg.add_calculation(ev.ADD, t, ev.vs(ev.FIXED, 0, lr[1]))
    return _program(k, _close(g, [a, ev.vs(ev.ADVICE, 3, rots[0])]), perm=4, lookup_graphs=[lg])


FORMS = [form_single_identity, form_empty_gates, form_horner_without_parts, form_bare_parts, form_zero_start_horner, form_same_value_twice, form_written_twice]


def _rotation_chain(g, rotations):
    """one column read per rotation, alternately added to and multiplied into a running value: every rotation is reachable from the result"""
    s = ev.vs(ev.FIXED, 0, g.add_rotation(rotations[0]))
    for i, r in enumerate(rotations[1:]):
        s = g.add_calculation(ev.ADD if i % 2 == 0 else ev.MUL, s, ev.vs(ev.ADVICE, i % 4, g.add_rotation(r)))
    return s


def rotations_program(k, gate_rotations, lookup_rotations=()):
    """a gate graph over `gate_rotations` and, if any, one lookup whose table expression reads `lookup_rotations`.  The lookup argument itself reads rotations 0, 1 and
    -1, which count towards the program's table of distinct rotations"""
    g = ev.Graph()
    s = _rotation_chain(g, list(gate_rotations))
    lgs = []
    if lookup_rotations:
        lg = ev.Graph()
        t = _rotation_chain(lg, list(lookup_rotations))
        lg.add_calculation(ev.ADD, t, ev.vs(ev.GAMMA))
        lgs.append(lg)
    return _program(k, _close(g, [s]), lookup_graphs=lgs)
