"""CPU tier of the sequence-set batches: exported symbols and struct layouts, pmx_all_pairs_count / pmx_all_pairs_index against
exact Python integers (every pair of small sets; the places where a rounded square root is off by one in large ones), the Python
restatement against brute force, and every refusal that needs no GPU (wrapped sets whose pointers are never followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seqset_create", "pmx_seqset_wrap_device", "pmx_seqset_free", "pmx_seqset_count", "pmx_align_pairs",
           "pmx_align_pairs_device", "pmx_all_pairs_count", "pmx_all_pairs_index", "pmx_align_all_pairs",
           "pmx_align_all_pairs_device", "pmx_all_pairs_enumerate_device")
NMAX = (1 << 31) - 1


def test_symbols_are_exported_and_declared(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert re.search(r"#define PMX_FLAG_BAD_PAIR 8\b", text)
    assert pkg.FLAG_BAD_PAIR == pairs_ref.FLAG_BAD_PAIR == 8


def test_pair_layout_matches_the_header_and_the_dtype(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    body = re.search(r"typedef struct pmx_pair \{(.*?)\} pmx_pair_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, fields = 0, []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        typ, names = decl.split(None, 1)
        size = {"int32_t": 4, "int64_t": 8}[typ]
        for name in names.split(","):
            off = (off + size - 1) // size * size
            fields.append((name.strip(), off, size))
            off += size
    assert off == 32 and C.sizeof(pkg.pmx_pair_t) == 32 and pkg.PAIR_DTYPE.itemsize == 32
    assert [f[0] for f in fields] == ["q", "r", "q_beg", "q_len", "r_beg", "r_len"]
    for name, o, size in fields:
        assert getattr(pkg.pmx_pair_t, name).offset == o and getattr(pkg.pmx_pair_t, name).size == size
        assert pkg.PAIR_DTYPE.fields[name][1] == o and pkg.PAIR_DTYPE.fields[name][0].itemsize == size
    assert pkg.PAIR_DTYPE == pairs_ref.PAIR_DTYPE
    assert C.sizeof(pkg.pmx_pairs_opts_t) == 8


def test_reference_index_equals_brute_force():
    for n in (2, 3, 4, 5, 17, 65):
        want = [(i, j) for i in range(n) for j in range(i + 1, n)]
        assert len(want) == pairs_ref.all_pairs_count(n)
        assert [pairs_ref.all_pairs_index(n, p) for p in range(len(want))] == want


def _index(pkg, n, p):
    i, j = C.c_int64(-7), C.c_int64(-7)
    assert pkg.lib.pmx_all_pairs_index(n, p, C.byref(i), C.byref(j)) == 0, (n, p)
    return i.value, j.value


@pytest.mark.parametrize("n", [2, 3, 4, 5, 65, 1000])
def test_all_pairs_index_every_pair(pkg, n):
    total = pkg.lib.pmx_all_pairs_count(n)
    assert total == pairs_ref.all_pairs_count(n) == pkg.all_pairs_count(n)
    want = [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert [_index(pkg, n, p) for p in range(total)] == want
    assert pkg.all_pairs_index(n, total - 1) == (n - 2, n - 1)


@pytest.mark.parametrize("n", [100000, NMAX])
def test_all_pairs_index_where_the_root_rounds(pkg, n):
    assert pkg.lib.pmx_all_pairs_count(n) == pairs_ref.all_pairs_count(n)
    rng = np.random.default_rng(6100 + n % 1000)
    ps = pairs_ref.edge_positions(n, rng)
    assert len(ps) >= 3 * 4096
    for p in ps:
        assert _index(pkg, n, p) == pairs_ref.all_pairs_index(n, p), (n, p)


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def _cfg(pkg, pm, want=0):
    return pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 0, want, pm.inner)


def test_count_and_index_refusals(pkg):
    L = pkg.lib
    assert L.pmx_all_pairs_count(0) == 0 and L.pmx_all_pairs_count(1) == 0 and L.pmx_all_pairs_count(2) == 1
    assert L.pmx_all_pairs_count(-1) == -1 and "nseq" in _err(pkg)
    assert L.pmx_all_pairs_count(NMAX + 1) == -1 and "2^31" in _err(pkg)
    i, j = C.c_int64(), C.c_int64()
    assert L.pmx_all_pairs_index(5, 10, C.byref(i), C.byref(j)) == -1 and "pair 10" in _err(pkg)
    assert L.pmx_all_pairs_index(5, -1, C.byref(i), C.byref(j)) == -1
    assert L.pmx_all_pairs_index(1, 0, C.byref(i), C.byref(j)) == -1
    assert L.pmx_all_pairs_index(NMAX + 1, 0, C.byref(i), C.byref(j)) == -1 and "nseq" in _err(pkg)
    assert L.pmx_all_pairs_index(5, 3, None, C.byref(j)) == -1 and "null" in _err(pkg)
    with pytest.raises(pkg.BatchError):
        pkg.all_pairs_index(5, 10)
    with pytest.raises(pkg.BatchError):
        pkg.all_pairs_count(-3)


def test_seqset_refusals(pkg):
    L = pkg.lib
    off = np.array([0, 4, 3], dtype=np.int64)
    buf = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    assert not L.pmx_seqset_create(buf.ctypes.data, None, 2) and "null" in _err(pkg)
    assert not L.pmx_seqset_create(None, off.ctypes.data, 2) and "null" in _err(pkg)
    assert not L.pmx_seqset_create(buf.ctypes.data, off.ctypes.data, -1) and "negative" in _err(pkg)
    assert not L.pmx_seqset_create(buf.ctypes.data, off.ctypes.data, 2) and "decrease at sequence 1" in _err(pkg)
    neg = np.array([-1, 4], dtype=np.int64)
    assert not L.pmx_seqset_create(buf.ctypes.data, neg.ctypes.data, 1) and "negative" in _err(pkg)
    assert not L.pmx_seqset_wrap_device(256, None, 2, 8) and "null" in _err(pkg)
    assert not L.pmx_seqset_wrap_device(None, 256, 2, 8)
    assert not L.pmx_seqset_wrap_device(256, 256, -1, 8)
    assert not L.pmx_seqset_wrap_device(256, 256, 2, -8)
    assert L.pmx_seqset_count(None) == -1
    L.pmx_seqset_free(None)
    s = pkg.SeqSet.wrap_device(256, 256, 7, 100)
    assert len(s) == 7
    s.close()
    s.close()
    with pytest.raises(pkg.BatchError):
        len(s)


def test_align_refusals_without_gpu(pkg):
    """wrapped sets over addresses that are never followed: every case ends before any GPU work"""
    L = pkg.lib
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    cfg = _cfg(pkg, pm)
    S = pkg.SeqSet.wrap_device(256, 256, 10, 1000)
    h = S.inner
    O = pkg.pmx_pairs_opts_t
    pairs = np.zeros(4, dtype=pkg.PAIR_DTYPE)
    out = np.zeros(64, dtype=pkg.RECORD_DTYPE)
    pp, po = pairs.ctypes.data, out.ctypes.data

    def host(c=cfg, q=h, r=h, n=4, p=pp, o=po, opts=None):
        return L.pmx_align_pairs(C.byref(c), q, r, n, p, o, None, C.byref(opts) if opts is not None else None)

    def dev(c=cfg, q=h, r=h, n=4, p=256, o=256, opts=None, mq=8, mr=8):
        return L.pmx_align_pairs_device(C.byref(c), q, r, n, p, mq, mr, o, None, None, C.byref(opts) if opts is not None else None)

    def all_host(c=cfg, s=h, first=0, count=4, o=po, opts=None):
        return L.pmx_align_all_pairs(C.byref(c), s, first, count, o, None, C.byref(opts) if opts is not None else None)

    def all_dev(c=cfg, s=h, first=0, count=4, o=256, opts=None, ml=8):
        return L.pmx_align_all_pairs_device(C.byref(c), s, first, count, ml, o, None, None, C.byref(opts) if opts is not None else None)

    for entry in (host, dev):
        assert entry(q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(p=None) == -1 and "null pairs" in _err(pkg)
        assert entry(o=None) == -1 and "null" in _err(pkg)
        assert entry(n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(opts=O(-1)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)) == -1 and "CIGAR" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_STATS)) == -1 and "stats" in _err(pkg)
        assert entry(c=pkg.pmx_config_t(7, 0, 5, 2, 0, 0, pm.inner)) == -1 and "mode" in _err(pkg)
        assert entry(n=0) == 0                                      # an empty batch touches nothing
        assert entry(n=0, p=None, o=None) == 0
    assert dev(mq=0) == -1 and "max_qlen" in _err(pkg)
    assert dev(mr=-5) == -1 and "max_qlen" in _err(pkg)
    total = pairs_ref.all_pairs_count(10)
    big = pkg.SeqSet.wrap_device(256, 256, NMAX + 1, 1000)
    for entry in (all_host, all_dev):
        assert entry(s=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(first=-1) == -1 and "negative" in _err(pkg)
        assert entry(count=-1) == -1 and "negative" in _err(pkg)
        assert entry(first=total - 3, count=4) == -1 and "beyond" in _err(pkg)
        assert entry(first=total + 1, count=0) == -1 and "beyond" in _err(pkg)
        assert entry(s=big.inner) == -1 and "nseq" in _err(pkg)
        assert entry(o=None) == -1 and "null" in _err(pkg)
        assert entry(opts=O(-2)) == -1 and "chunk_pairs" in _err(pkg)
        assert entry(c=_cfg(pkg, pm, pkg.WANT_CIGAR)) == -1 and "CIGAR" in _err(pkg)
        assert entry(count=0) == 0
        assert entry(first=total, count=0) == 0
    assert all_dev(ml=0) == -1 and "positive" in _err(pkg)
    assert L.pmx_all_pairs_enumerate_device(NMAX + 1, 0, 4, 256, None) == -1 and "nseq" in _err(pkg)
    assert L.pmx_all_pairs_enumerate_device(10, total - 1, 2, 256, None) == -1 and "beyond" in _err(pkg)
    assert L.pmx_all_pairs_enumerate_device(10, -1, 2, 256, None) == -1
    assert L.pmx_all_pairs_enumerate_device(10, 0, 2, None, None) == -1 and "null" in _err(pkg)
    assert L.pmx_all_pairs_enumerate_device(10, 0, 0, None, None) == 0


def test_python_mirror_refuses_a_profile_and_builds_descriptors(pkg):
    pm = pkg.Matrix.create(b"ACGT", 2, -3)
    al = pkg.Aligner.new().local().matrix(pm).profile(pkg.Profile.new(b"ACGT", False, pm)).build()
    S = pkg.SeqSet.wrap_device(256, 256, 3, 12)
    with pytest.raises(pkg.BatchError):
        al.align_pairs(S, S, [(0, 1)])
    with pytest.raises(pkg.BatchError):
        al.align_all_pairs(S)
    a = pkg.as_pairs([(0, 1), (2, 1, 3, 4, 5, -1)])
    assert a.dtype == pkg.PAIR_DTYPE and a.tolist() == [(0, 1, 0, -1, 0, -1), (2, 1, 3, 4, 5, -1)]
    assert a.tolist() == pairs_ref.pairs_array([(0, 1), (2, 1, 3, 4, 5, -1)]).tolist()


@pytest.mark.gpu                      # the refusals happen before any GPU work, but a set with host offsets is uploaded when it is created
def test_lowest_bad_pair_across_the_slices_of_the_scan(pkg):
    """262 144 + 3 listed pairs are scanned in four slices on helper threads: the pair named is the lowest bad one of the list,
    whichever slice found it, on the plain host entry and on a frameshift one; a window without a codon below it is named first"""
    rng = np.random.default_rng(6200)
    n, nseq = 262144 + 3, 16
    S = pkg.SeqSet.new([bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=8)) for _ in range(nseq)])
    pairs = np.zeros(n, dtype=pkg.PAIR_DTYPE)
    pairs["q"], pairs["r"] = rng.integers(0, nseq, size=n), rng.integers(0, nseq, size=n)
    pairs["q_len"] = pairs["r_len"] = -1
    plain = pkg.Aligner.new().local().matrix(pkg.Matrix.create(b"ACGT", 2, -3)).gap_open(5).gap_extend(2).build()
    shift = pkg.Aligner.new().local().matrix(pkg.Matrix.from_name("blosum62")).gap_open(11).gap_extend(1).build()
    entries = (lambda p: plain.align_pairs(S, S, p), lambda p: shift.align_pairs(S, S, p, frameshift=4, strand="both"))
    last, second = n - 1000, n // 4 + 5
    assert last >= n * 3 // 4 and n // 4 <= second < n // 2
    pairs[last]["r"] = nseq                                         # the last quarter: the fourth slice
    for entry in entries:
        with pytest.raises(pkg.BatchError, match=r"^pair %d: reference: index outside the set$" % last):
            entry(pairs)
    pairs[second]["q_beg"] = 7; pairs[second]["q_len"] = 2          # the second quarter: the second slice
    for entry in entries:
        with pytest.raises(pkg.BatchError, match=r"^pair %d: query: window reaches past the end of the sequence$" % second):
            entry(pairs)
    pairs[100]["q_beg"] = 3; pairs[100]["q_len"] = 2                # a good descriptor whose W < 3, below both
    with pytest.raises(pkg.BatchError, match=r"^pair 100: query: a window of 2 nucleotides has no codon$"):
        entries[1](pairs)
    with pytest.raises(pkg.BatchError, match=r"^pair %d: query: window reaches past" % second):
        entries[0](pairs)                                           # (the plain entry takes a window of two letters)
