"""The unit programs of the latency path (bls_amd/csrc/gen_lat.py: UNIT_PROGRAMS) for the tests: the scheduled programs, the tuples of raw
operands they run on, and what every output must be -- Python integers straight from the job table, with the formulas of the job kinds:

    MUL  (sum c_i a_i)(sum d_j b_j) / R      SQR  3 x^2 / R      LIN  sum c_i a_i      INV  x^-1 R^2 (0 for 0)        mod q, R = 2^405

(values are those of the device representation: the integer the 15 limbs hold).  An un-reduced LIN job keeps the INTEGER sum -- the limb
normalisation moves carries, nothing else -- so over inputs and other un-reduced LIN results the expectation is exact, not modulo q.  A plain
module, shared by tests/test_lat_units_cpu.py and tests/test_gpu_lat_units.py; no GPU."""
import functools
import importlib.util
import os

import lat_operands as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_lat", os.path.join(ROOT, "bls_amd", "csrc", "gen_lat.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

Q = G.Q
R = G.RMONT
RINV = pow(R, -1, Q)
# programs whose x-side operands read inputs 0..7 and y-side operands inputs 8..15; the others have one side, split in halves for the sign tuples
TWO_SIDED = ("unit_mul0", "unit_mul1", "unit_mul2", "unit_mulv")


@functools.lru_cache(maxsize=None)
def program(name):
    return G.schedule(G.build_unit_program(name))


def which(name):
    return G.UNIT_PROGRAMS.index(name)


def nin(name):
    return len(program(name).inputs)


def nout(name):
    """result elements that leave as limbs (0: a verdict program)"""
    p = program(name)
    return len(p.out_nodes) if p.out == "outraw12" else 0


def level_reduces(jobs):
    """the value reduction of a LIN level is level-wide (gen_lat.py encode): one job that asks for it reduces all"""
    return any(n.reduce for n in jobs)


def evaluate(p, raw_values):
    """raw_values: the integer value of every input element.  -> per output node (class, value mod q, exact integer or None), class in
    'prod' (MUL / SQR), 'lin' (un-reduced LIN), 'red' (LIN of a reducing level), 'inv'"""
    mod, exact, cls = {}, {}, {}
    for n in p.consts:
        mod[n.id] = exact[n.id] = n.aux * R % Q                          # constants: canonical limbs of the Montgomery form
    def ev(lin, table):
        return sum(c * table[d.id] for d, c in lin.items())
    for kind, jobs in p.levels:
        red = kind == G.K_LIN and level_reduces(jobs)
        for n in jobs:
            ex = None
            if n.kind == "in":
                ex = raw_values[n.aux[1]]; v = ex % Q; c = "in"
            elif n.kind == "mul":
                v = ev(n.x, mod) * ev(n.y, mod) * RINV % Q; c = "prod"
            elif n.kind == "sqr3":
                x = ev(n.x, mod); v = 3 * x * x * RINV % Q; c = "prod"
            elif n.kind == "lin":
                v = ev(n.x, mod) % Q
                if not red and all(exact.get(d.id) is not None for d in n.x):
                    ex = ev(n.x, exact)
                c = "red" if red else "lin"
            elif n.kind == "inv":
                x = ev(n.x, mod) % Q; v = pow(x, -1, Q) * R * R % Q if x else 0; c = "inv"
            else:
                raise AssertionError(n.kind)
            mod[n.id], exact[n.id], cls[n.id] = v, ex, c
    return [(cls[n.id], mod[n.id], exact[n.id]) for n in p.out_nodes]


def _sides(name):
    k = nin(name)
    nx = 8 if name in TWO_SIDED else (k + 1) // 2
    return nx, k - nx


def tuples(name):
    """the tuples (lists of nin raw representatives) a unit program runs on, an odd count: the sign patterns at the limb bound, the values
    within eps of +-q (real magnitudes then reach the nominal value bounds), and the corpus walked through every input position"""
    k = nin(name)
    nx, ny = _sides(name)
    both = lambda x, y: [x] * nx + [y] * ny
    t = [both(O.ALL_PLUS, O.ALL_PLUS), both(O.neg(O.ALL_PLUS), O.neg(O.ALL_PLUS)), both(O.ALL_PLUS, O.neg(O.ALL_PLUS)), both(O.neg(O.ALL_PLUS), O.ALL_PLUS),
         both(O.ALL_MINUS, O.ALL_MINUS), both(O.ALL_PLUS, O.ALL_MINUS), both(O.ALT0, O.ALT0), both(O.ALT1, O.ALT1), both(O.ALT0, O.ALT1), both(O.ALT0, O.neg(O.ALT0)),
         [O.ALT0 if i % 2 == 0 else O.ALT1 for i in range(k)], [O.ALL_PLUS if i % 2 == 0 else O.neg(O.ALL_PLUS) for i in range(k)]]
    for p, m in zip(O.NEAR_Q, O.NEAR_Q_NEG):
        t += [both(p, p), both(m, m), both(p, m)]
    c = O.CORPUS
    t += [[c[(j + 5 * i) % len(c)] for i in range(k)] for j in range(len(c))]
    if name in ("unit_check1", "unit_iszero"):
        z, o = O.ZERO_REPS, O.ONE_REPS
        for j in range(len(z) * len(o)):
            zeros = [z[(j + i) % len(z)] for i in range(k)]
            first = o[j % len(o)]
            t += [[first] + zeros[1:], zeros, zeros[:5] + [first] + zeros[6:], [O.canon(1)] + zeros[1:], zeros[:11] + [O.canon(1)],
                  [first] + zeros[1:7] + [O.neg(O.canon(1))] + zeros[8:], [O.neg(first)] + zeros[1:]]
    if len(t) % 2 == 0:
        t.append([c[(7 * i + 3) % len(c)] for i in range(k)])
    assert len(t) <= 513 and all(len(x) == k for x in t)
    return t
