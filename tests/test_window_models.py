"""CPU tier: the stored-arithmetic model of the packed global / semi-global kernels (tests/nwsgv_model.c) at the corners of the host's
range proof (`pmx_nwsgv_bias`, exported as the test hook `pmx_window_nwsgv`).

pmx_nwsg16.hip has no promotion pass: a batch the predicate admits must keep EVERY stored 16-bit pattern inside [1024, 31743].  The
round-3 soak found a window bug (fuzz seed 5018: the last-column capture left the window) that no CPU-tier test could have caught.
The model replays the kernel's stored form lane for lane -- bias, column skew, row offsets, virtual rows and columns, captures -- and
counts what leaves its domain; here it runs on the inputs that stretch the range (all matches, no match, a copy behind a long gap,
poly-A) at the LONGEST reference the predicate admits per scoring scheme and shape, and one column short of it."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from util import B62_LETTERS, consensus_pssm, random_seqs

HERE = os.path.dirname(os.path.abspath(__file__))


class Out(C.Structure):
    _fields_ = [("score", C.c_int), ("end_query", C.c_int), ("end_ref", C.c_int), ("lo", C.c_int), ("hi", C.c_int),
                ("violations", C.c_int), ("first_violation_kind", C.c_int), ("dmin", C.c_int), ("dmax", C.c_int), ("diff_violations", C.c_int)]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nwsgv_model") / "nwsgv_model.so")
    subprocess.run(["gcc", "-O3", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "nwsgv_model.c")], check=True)
    lib = C.CDLL(so)
    lib.nwsgv_model.restype = C.c_int
    return lib


def _window(pkg, qlen, rlen, smin, smax, open_, ext, rowx, rows, msize=5):
    pkg.lib.pmx_window_nwsgv.restype = C.c_int
    return pkg.lib.pmx_window_nwsgv(qlen, rlen, msize, smin, smax, open_, ext, rowx, rows)


def _run_mat(model, G, R, rowx, top, legacy, pssm, qi, ri, max_rlen, mat, msize, open_, ext, sg, nb):
    """qi, ri: mapped symbols (uint8); mat: int32 [msize, msize], or with pssm [len(qi), msize] (qi then only gives the length)"""
    mat = np.ascontiguousarray(mat, dtype=np.int32)
    qi, ri = np.ascontiguousarray(qi, dtype=np.uint8), np.ascontiguousarray(ri, dtype=np.uint8)
    assert mat.shape == ((len(qi) if pssm else msize), msize)
    out = Out()
    col_pen, row_pen = int(not (sg & 1)), int(not (sg & 4))
    rc = model.nwsgv_model(G, R, rowx, top, legacy, pssm, qi.ctypes.data_as(C.c_void_p), len(qi), ri.ctypes.data_as(C.c_void_p), len(ri), max_rlen,
                           mat.ctypes.data_as(C.c_void_p), msize, open_, ext, col_pen, row_pen, int(bool(sg & 2)), int(bool(sg & 8)), nb, C.byref(out))
    assert rc == 0
    return out


def _run(model, G, R, rowx, top, legacy, q, r, max_rlen, om, open_, ext, sg, nb):
    return _run_mat(model, G, R, rowx, top, legacy, 0, _LUT[np.frombuffer(q, dtype=np.uint8)], _LUT[np.frombuffer(r, dtype=np.uint8)], max_rlen,
                    om.scores[:5, :5], 5, open_, ext, sg, nb)


_LUT = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i
_ROT = bytes.maketrans(b"ACGT", b"CGTA")


def _oracle(orc, q, r, om, open_, ext, sg):
    qb, qo = orc.pack([q]); rb, ro = orc.pack([r])
    mode = orc.NW if sg == 0 else orc.SG
    return tuple(int(x) for x in orc.align_batch(mode, qb, qo, rb, ro, open_, ext, om, sg_flags=sg if sg else orc.SG_ALL)[0])


SHAPES = [(8, 7), (8, 16), (16, 10), (16, 16), (32, 10), (64, 2), (64, 16), (8, 20)]


def test_model_matches_the_oracle_on_small_pairs(orc, pkg, model):
    """both alignments of the query in the shape (virtual rows on top / padding rows below), with and without the row offset, every
    free-end set: same score and end positions as the oracle, nothing outside its domain"""
    rng = np.random.default_rng(4100)
    n = 0
    for it in range(160):
        G, R = SHAPES[int(rng.integers(0, len(SHAPES)))]
        match, mis = [(2, -3), (5, -4), (1, -1), (3, -2), (9, -9)][int(rng.integers(0, 5))]
        open_, ext = [(5, 2), (1, 1), (10, 1), (4, 4), (3, 0), (0, 0), (20, 3)][int(rng.integers(0, 7))]
        om = orc.Matrix.create("ACGT", match, mis)
        qlen = int(rng.choice([1, 2, G * R, G * R - 1, int(rng.integers(1, G * R + 1))]))
        rlen = int(rng.choice([1, 2, 17, int(rng.integers(1, 200))]))
        q, r = random_seqs(rng, 1, qlen, qlen)[0], random_seqs(rng, 1, rlen, rlen)[0]
        if rng.random() < 0.5:
            r = (q * (rlen // qlen + 1))[:rlen]
        sg = int(rng.integers(0, 16))
        for rowx in (1, 0):
            nb = _window(pkg, qlen, rlen, mis, match, open_, ext, rowx, G * R)
            if not nb:
                continue
            for top in (0, 1):
                out = _run(model, G, R, rowx, top, 0, q, r, rlen + int(rng.integers(0, 40)), om, open_, ext, sg, nb)
                want = _oracle(orc, q, r, om, open_, ext, sg)
                assert (out.score, out.end_query, out.end_ref) == want and out.violations == 0, \
                    (G, R, rowx, top, match, mis, open_, ext, sg, qlen, rlen, (out.score, out.end_query, out.end_ref), want, out.violations, out.lo, out.hi)
                n += 1
    assert n > 400, n


@pytest.mark.parametrize("rowx", [1, 0])
def test_nothing_leaves_the_window_at_the_longest_reference_the_proof_admits(orc, pkg, model, rowx):
    rng = np.random.default_rng(4200 + rowx)
    n = 0
    tightest = 0
    for match, mis, open_, ext in ((2, -3, 5, 2), (1, -1, 1, 1), (5, -4, 10, 1), (3, -2, 4, 4), (9, -9, 20, 3), (1, -30, 60, 1), (2, -3, 120, 5)):
        om = orc.Matrix.create("ACGT", match, mis)
        for G, R in ((8, 7), (16, 16), (64, 2)) + (((64, 16),) if ext == 2 else ()):
            for qlen in sorted({1, min(50, G * R), G * R}):
                lo, hi = 0, 30000
                if not _window(pkg, qlen, 1, mis, match, open_, ext, rowx, G * R):
                    continue
                lo = 1
                while hi - lo > 0:                                  # the longest reference the predicate admits for this shape
                    mid = (lo + hi + 1) // 2
                    lo, hi = (mid, hi) if _window(pkg, qlen, mid, mis, match, open_, ext, rowx, G * R) else (lo, mid - 1)
                for rlen in sorted({lo, max(1, lo - 1)}):
                    if qlen * rlen > 9_000_000:
                        continue                                    # (kept to sizes the scalar oracle does in a blink)
                    nb = _window(pkg, qlen, rlen, mis, match, open_, ext, rowx, G * R)
                    assert nb
                    q0 = random_seqs(rng, 1, qlen, qlen)[0]
                    far = random_seqs(rng, 1, rlen, rlen)[0]
                    refs = [(q0 * (rlen // qlen + 1))[:rlen],
                            (q0 * (rlen // qlen + 1))[:rlen].translate(_ROT),
                            (far[:rlen - qlen] + q0) if rlen > qlen else far, (q0 + far[:rlen - qlen]) if rlen > qlen else far]
                    for r, q in [(x, q0) for x in (refs if rlen == lo else refs[::2])] + [(b"A" * rlen, b"A" * qlen)]:
                        for sg in ((0, 15, 10, 5) if rlen == lo else (2, 8)):
                            for top in (0, 1):
                                out = _run(model, G, R, rowx, top, 0, q, r, rlen, om, open_, ext, sg, nb)
                                assert out.violations == 0, ("outside its domain", out.first_violation_kind, out.lo, out.hi, G, R, top, match, mis, open_, ext, sg, qlen, rlen)
                                tightest = max(tightest, out.hi)
                                if top == 0 and n % 16 == 0:         # (the oracle on a sample: the values are what this test is about)
                                    want = _oracle(orc, q, r, om, open_, ext, sg)
                                    assert (out.score, out.end_query, out.end_ref) == want, (G, R, match, mis, open_, ext, sg, qlen, rlen, want)
                                n += 1
    assert n > 1000, n
    assert tightest > 24000, tightest                               # the corners really are close to the top of the window


def test_the_model_flags_the_capture_form_the_round_3_soak_caught(orc, pkg, model):
    """(fuzz seed 5018) the last-column capture once compared the rows with their offsets taken off and the capture bias added: a short
    query against a reference of tens of kilobases under extend = 1 with a free query end left the window.  The model, run with that
    form, flags exactly that operand; with the form the kernels use now it is clean on the same input."""
    om = orc.Matrix.create("ACGT", 2, -3)
    rng = np.random.default_rng(5018)
    G, R, qlen, open_, ext = 8, 7, 50, 5, 1
    flagged = clean = 0
    for rlen in (18000, 22000, 26000, 28000):
        nb = _window(pkg, qlen, rlen, -3, 2, open_, ext, 1, G * R)
        if not nb:
            continue
        q = random_seqs(rng, 1, qlen, qlen)[0]
        r = random_seqs(rng, 1, rlen - qlen, rlen - qlen)[0] + q
        for sg in (2, 10, 15):
            old = _run(model, G, R, 1, 0, 1, q, r, rlen, om, open_, ext, sg, nb)
            new = _run(model, G, R, 1, 0, 0, q, r, rlen, om, open_, ext, sg, nb)
            flagged += int(old.violations > 0 and old.first_violation_kind == 4)
            clean += int(new.violations == 0 and (new.score, new.end_query, new.end_ref) == _oracle(orc, q, r, om, open_, ext, sg))
    assert flagged >= 3 and clean >= 9, (flagged, clean)


# ---------------------------------------------------------------------------------------------------------------------------------
# The shared-profile (pmx_nwsg16q_kernel, symbol and PSSM forms) and matrix-lookup (pmx_nwsg16m_kernel) kernels run the same stored
# arithmetic on the same proof with a 24-letter matrix; their traceback instances add the bounded-difference decision merge.

# every shape the shared-profile / matrix-lookup ladders pick, and the two trace-only shapes (a trace shape keeps one virtual row)
LADDER = [(16, 10), (16, 16), (32, 10), (32, 16), (64, 16), (64, 32)]
TRACE_ONLY = [(16, 19), (16, 20)]
GAPS = [(11, 1), (10, 2), (5, 2), (20, 3), (11, 11)]


def _b62(orc):
    from util import golden
    om = orc.Matrix.from_file(golden("blosum62.txt"))
    assert om.size == 24 and int(om.scores.min()) == -4 and int(om.scores.max()) == 11
    return om


def _longest(pkg, qlen, smin, smax, open_, ext, rows, msize=24):
    """the longest reference pmx_window_nwsgv admits (row-offset form) -- it must admit a reference of one letter"""
    assert _window(pkg, qlen, 1, smin, smax, open_, ext, 1, rows, msize), ("refused at reference length 1", qlen, smin, smax, open_, ext, rows)
    lo, hi = 1, 30000
    while hi - lo > 0:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if _window(pkg, qlen, mid, smin, smax, open_, ext, 1, rows, msize) else (lo, mid - 1)
    return lo


def _run_all(model, jobs):
    """jobs: the arguments of _run_mat behind `model`; ctypes releases the interpreter lock for the model's run, so a few threads
    work side by side.  Results in the jobs' order."""
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(lambda a: _run_mat(model, *a), jobs))


def _square_oracle(orc, om, q, r, open_, ext, sg):
    qb, qo = orc.pack([q]); rb, ro = orc.pack([r])
    return tuple(int(x) for x in orc.align_batch(orc.NW if sg == 0 else orc.SG, qb, qo, rb, ro, open_, ext, om, sg_flags=sg if sg else orc.SG_ALL, bits=32)[0])


def _qlens(G, R, trace_only):
    return sorted({min(50, G * R - 1), G * R - 1} | (set() if trace_only else {G * R}))


def _corner_modes(at_longest):
    return (0, 15, 10, 5) if at_longest else (2, 8)


def test_blosum62_at_the_window_edge(orc, pkg, model):
    """BLOSUM62 (24 letters, -4 .. 11) in every shape of the shared-profile and matrix-lookup ladders and the trace shapes, five gap
    models, at the longest reference pmx_window_nwsgv admits for that shape's rows and one column short of it: poly-W against
    poly-W (the steepest climb), the query repeated, the query behind a long unrelated prefix, W against '*' (the steepest
    descent) and a random pair.  Nothing leaves the window, no decision difference leaves [-256, 255] (11 + 2 * 20 <= 250), and
    the model's result equals the oracle's on every 16th run.  Measured: the tightest stored pattern is 31 127 of 31 743."""
    from util import AA
    om = _b62(orc)
    rng = np.random.default_rng(4300)
    lut = om.mapper.astype(np.uint8)
    jobs, meta = [], []
    for open_, ext in GAPS:
        for G, R in LADDER + TRACE_ONLY:
            for qlen in _qlens(G, R, (G, R) in TRACE_ONLY):
                longest = _longest(pkg, qlen, -4, 11, open_, ext, G * R)
                for rlen in sorted({longest, max(1, longest - 1)}):
                    nb = _window(pkg, qlen, rlen, -4, 11, open_, ext, 1, G * R, 24)
                    assert nb
                    q0 = random_seqs(rng, 1, qlen, qlen, AA)[0]
                    far = random_seqs(rng, 1, rlen, rlen, AA)[0]
                    pairs = [(b"W" * qlen, b"W" * rlen), (q0, (q0 * (rlen // qlen + 1))[:rlen]),
                             (q0, far[:rlen - qlen] + q0 if rlen > qlen else far), (b"W" * qlen, b"*" * rlen), (q0, far)]
                    for q, r in (pairs if rlen == longest else pairs[:4:3] + pairs[2:3]):
                        for sg in _corner_modes(rlen == longest):
                            jobs.append((G, R, 1, 0, 0, 0, lut[np.frombuffer(q, dtype=np.uint8)], lut[np.frombuffer(r, dtype=np.uint8)],
                                         rlen, om.scores, 24, open_, ext, sg, nb))
                            meta.append((q, r))
    n = compared = tightest = 0
    for job, (q, r), out in zip(jobs, meta, _run_all(model, jobs)):
        G, R, open_, ext, sg = job[0], job[1], job[11], job[12], job[13]
        assert out.violations == 0 and out.diff_violations == 0, \
            ("outside its domain", out.first_violation_kind, out.lo, out.hi, out.dmin, out.dmax, G, R, open_, ext, sg, len(q), len(r))
        tightest = max(tightest, out.hi)
        if n % 16 == 0:
            want = _square_oracle(orc, om, q, r, open_, ext, sg)
            assert (out.score, out.end_query, out.end_ref) == want, (G, R, open_, ext, sg, len(q), len(r), want)
            compared += 1
        n += 1
    print("blosum62 window edge: runs %d, compared with the oracle %d, tightest hi %d" % (n, compared, tightest))
    assert n > 2500 and compared > 150, (n, compared)
    assert tightest > 24000, tightest


def _pssm_oracle(orc, vals, square, q, r, b62_mapper, open_, ext, sg):
    if square is not None:
        return _square_oracle(orc, orc.Matrix(square, b62_mapper), q, r, open_, ext, sg)
    from pssm_oracle import encode
    om, qcode = encode(orc, vals, b62_mapper, B62_LETTERS)
    return _square_oracle(orc, om, qcode, r, open_, ext, sg)


@pytest.mark.parametrize("case", ["A", "B"])
def test_pssms_at_the_window_edge(orc, pkg, model, case):
    """PSSM rows (the model's pssm flag = PSSM = true of pmx_nwsg16q_kernel) whose every row holds its top value in its consensus
    column, same corners as the BLOSUM62 test.  A: top 255 - open - ext (the largest profile byte) and -open under '*' (byte 0) --
    short admitted references, the steepest climb per column; B: a mild PSSM (-6 .. 9) with long references.  Up to 200 rows the
    PSSM is random per row and the byte-encoded checker's matrix is the oracle; beyond, rows of equal query letters are equal and
    the square oracle scores them.  The references: the consensus repeated, the consensus behind a long prefix, poly-'*', random.
    Measured: the tightest stored pattern is 30 663 (A) and 31 131 (B) of 31 743."""
    from util import AA
    b62map = _b62(orc).mapper
    lut = b62map.astype(np.uint8)
    rng = np.random.default_rng(4400 + ord(case))
    jobs, meta = [], []
    for open_, ext in GAPS:
        low = max(-6, -open_)                                        # (a profile byte score + open must not fall below 0)
        top, bottom = (255 - open_ - ext, -open_) if case == "A" else (9, low)
        gate = top + 2 * open_ <= 250
        for G, R in LADDER + TRACE_ONLY:
            for L in _qlens(G, R, (G, R) in TRACE_ONLY):
                q = random_seqs(rng, 1, L, L, AA)[0]
                vals, cons, square = consensus_pssm(rng, L, top, bottom, lo=low, by_letter=q if L > 200 else None)
                smin, smax = int(vals.min()), int(vals.max())
                assert (smin, smax) == (min(bottom, low), top)
                longest = _longest(pkg, L, smin, smax, open_, ext, G * R)
                for rlen in sorted({longest, max(1, longest - 1)}):
                    nb = _window(pkg, L, rlen, smin, smax, open_, ext, 1, G * R, 24)
                    assert nb
                    far = random_seqs(rng, 1, rlen, rlen, AA)[0]
                    refs = [(cons * (rlen // L + 1))[:rlen], far[:rlen - L] + cons if rlen > L else far, b"*" * rlen, far]
                    for r in (refs if rlen == longest else refs[:3]):
                        for sg in _corner_modes(rlen == longest):
                            jobs.append((G, R, 1, 0, 0, 1, np.zeros(L, dtype=np.uint8), lut[np.frombuffer(r, dtype=np.uint8)],
                                         rlen, vals, 24, open_, ext, sg, nb))
                            meta.append((q, r, square, gate))
    n = compared = tightest = 0
    for job, (q, r, square, gate), out in zip(jobs, meta, _run_all(model, jobs)):
        G, R, vals, open_, ext, sg = job[0], job[1], job[9], job[11], job[12], job[13]
        assert out.violations == 0 and (out.diff_violations == 0 or not gate), \
            ("outside its domain", out.first_violation_kind, out.lo, out.hi, out.dmin, out.dmax, G, R, open_, ext, sg, len(q), len(r))
        tightest = max(tightest, out.hi)
        if n % 16 == 0:
            want = _pssm_oracle(orc, vals, square, q, r, b62map, open_, ext, sg)
            assert (out.score, out.end_query, out.end_ref) == want, (G, R, open_, ext, sg, len(q), len(r), want)
            compared += 1
        n += 1
    print("pssm window edge %s: runs %d, compared with the oracle %d, tightest hi %d" % (case, n, compared, tightest))
    assert n > 2000 and compared > 120, (n, compared)
    assert tightest > 24000, tightest


# (match, mismatch, open) with max + 2 open == 250: the host's gate for the one-instruction decision merge
GATE_SCHEMES = [(110, -70, 70), (40, -105, 105), (248, -1, 1), (228, -11, 11), (250, 0, 0)]
GATE_SHAPES = [(16, 16), (8, 16)]


def gate_exts_required(open_):
    """the ext values that MUST run in every shape: for the gate's small pairs the window proof admits 0, 1 and open / 2 under
    every scheme; ext = open only while open is small (with open = 70 or 105 the skew growth (rlen + rows + 132) * ext passes the
    int16 window for all but the shortest references -- such runs are checked where they occur)"""
    return {0, 1, open_ // 2} & set(range(open_ + 1)) | ({open_} if open_ <= 11 else set())


def gate_exts(open_):
    return sorted({0, 1, open_ // 2, open_} & set(range(open_ + 1)))


def _gate_pairs(rng, G, R, count=40):
    """small random and repeated pairs, ragged"""
    out = []
    for k in range(count):
        qlen = int(rng.choice([1, 2, 17, G * R - 1, int(rng.integers(1, G * R))]))
        rlen = int(rng.choice([1, 3, 40, int(rng.integers(1, 120))]))
        q = random_seqs(rng, 1, qlen, qlen)[0]
        r = (q * (rlen // qlen + 1))[:rlen] if k % 2 else random_seqs(rng, 1, rlen, rlen)[0]
        out.append((q, r))
    return out


def _gate_sweep(orc, pkg, model, rng, match, mis, open_, compare):
    """every admitted ext x shape x pair x a free-end set through the model: per ext and shape [runs, smallest, largest difference,
    violations]"""
    om = orc.Matrix.create("ACGT", match, mis)
    smin, smax = int(om.scores[:5, :5].min()), int(om.scores[:5, :5].max())
    res = {}
    for ext in gate_exts(open_):
        for G, R in GATE_SHAPES:
            acc = res.setdefault((ext, G, R), [0, 1 << 30, -(1 << 30), 0])
            for k, (q, r) in enumerate(_gate_pairs(rng, G, R)):
                nb = _window(pkg, len(q), len(r), smin, smax, open_, ext, 1, G * R)
                if not nb:
                    continue                                         # (the window closes first, e.g. ext = open = 105: counted by the caller)
                sg = (0, 15, 5, 10, 2, 8)[k % 6]
                for top in (0, 1):
                    out = _run(model, G, R, 1, top, 0, q, r, len(r), om, open_, ext, sg, nb)
                    assert out.violations == 0, (match, mis, open_, ext, G, R, top, sg, out.first_violation_kind, out.lo, out.hi)
                    if compare:
                        assert (out.score, out.end_query, out.end_ref) == _oracle(orc, q, r, om, open_, ext, sg), (match, mis, open_, ext, G, R, top, sg, q, r)
                    acc[0] += 1; acc[1] = min(acc[1], out.dmin); acc[2] = max(acc[2], out.dmax); acc[3] += out.diff_violations
    return res


def _gate_pssm_sweep(orc, pkg, model, rng, top, open_, compare):
    from util import AA
    from pssm_oracle import encode
    b62map = _b62(orc).mapper
    lut = b62map.astype(np.uint8)
    res = {}
    for ext in gate_exts(open_):
        for G, R in ((16, 16), (16, 19)):
            acc = res.setdefault((ext, G, R), [0, 1 << 30, -(1 << 30), 0])
            for k in range(12):
                L = int(rng.choice([1, 2, 60, 200]))
                vals, cons, _ = consensus_pssm(rng, L, top, -open_, lo=max(-6, -open_), hi=min(9, top))     # (the profile byte score + open must not go below 0)
                rlen = int(rng.integers(1, 120))
                r = [(cons * (rlen // L + 1))[:rlen], random_seqs(rng, 1, rlen, rlen, AA)[0], b"*" * rlen][k % 3]
                nb = _window(pkg, L, rlen, int(vals.min()), int(vals.max()), open_, ext, 1, G * R, 24)
                if not nb:
                    continue
                sg = (0, 15, 5, 10, 2, 8)[k % 6]
                out = _run_mat(model, G, R, 1, 0, 0, 1, np.zeros(L, dtype=np.uint8), lut[np.frombuffer(r, dtype=np.uint8)], rlen, vals, 24, open_, ext, sg, nb)
                assert out.violations == 0, (top, open_, ext, G, R, sg, out.first_violation_kind, out.lo, out.hi)
                if compare:
                    om, qcode = encode(orc, vals, b62map, B62_LETTERS)
                    assert (out.score, out.end_query, out.end_ref) == _square_oracle(orc, om, qcode, r, open_, ext, sg), (top, open_, ext, G, R, sg, L, rlen)
                acc[0] += 1; acc[1] = min(acc[1], out.dmin); acc[2] = max(acc[2], out.dmax); acc[3] += out.diff_violations
    return res


def test_the_bounded_difference_gate_holds_and_is_tight(orc, pkg, model):
    """The one-instruction decision merge (v_bfi_b32 of the TRB form of pmx_nwsg16v_kernel and of every traceback instance of
    pmx_nwsg16q_kernel) needs T - H, F - H, E - X and F - X inside [-256, 255]; the host admits it while max(matrix max, 0) +
    2 open <= 250.  At exactly 250 -- symbol schemes and PSSMs with top 250 - 2 open and bottom -open -- no difference leaves the
    range, the smallest one observed is <= -(max + 2 open) (the bound is reached by ordinary small pairs: no sub-case is vacuous)
    and the model's results equal the oracle's.  Then max is raised one unit at a time with open fixed for as long as the window
    proof admits the scheme (248/-1/1 and 250/0/0 leave it first: the profile byte max + open + ext passes 255).  Measured: the
    first max + 2 open at which a difference leaves [-256, 255] is 257 (smallest difference -257), for 110/-70/70, 40/-105/105
    and 228/-11/11 alike -- the smallest difference is exactly -(max + 2 open), and the gate of 250 stops six units short of
    where the merge breaks."""
    rng = np.random.default_rng(4500)

    def at_the_gate(what, open_, res):
        # no sub-case is vacuous: every required ext value ran in every shape, and reached the bound there
        for (ext, G, R), (runs, dmin, dmax, bad) in sorted(res.items()):
            print("gate %s ext %d <%d,%d>: runs %d, differences %d .. %d" % (what, ext, G, R, runs, dmin, dmax))
            if ext in gate_exts_required(open_):
                assert runs >= 8 and dmin <= -250, (what, ext, G, R, runs, dmin)
            if runs:
                assert bad == 0 and -256 <= dmin and dmax <= 255, (what, ext, G, R, runs, dmin, dmax, bad)
    for match, mis, open_ in GATE_SCHEMES:
        assert match + 2 * open_ == 250
        at_the_gate("%d/%d/%d" % (match, mis, open_), open_, _gate_sweep(orc, pkg, model, rng, match, mis, open_, True))
    for open_ in (70, 105, 1, 11, 0):
        at_the_gate("pssm top %d open %d" % (250 - 2 * open_, open_), open_, _gate_pssm_sweep(orc, pkg, model, rng, 250 - 2 * open_, open_, True))
    first = {}
    for match, mis, open_ in GATE_SCHEMES:
        for over in range(1, 40):
            res = _gate_sweep(orc, pkg, model, rng, match + over, mis, open_, False)
            if sum(v[0] for v in res.values()) == 0:
                break                                                # (the profile byte max + open + ext passed 255: the window proof refuses the scheme)
            if sum(v[3] for v in res.values()):
                first[(match, mis, open_)] = (250 + over, min(v[1] for v in res.values()))
                break
    print("first max + 2 open with a difference outside [-256, 255]:", first)
    assert first, "no scheme could be raised past the gate inside the window proof"
    assert min(v[0] for v in first.values()) >= 251, first
    assert min(v[0] for v in first.values()) == 257, first         # (the measured value the docstring and DESIGN.md quote)
