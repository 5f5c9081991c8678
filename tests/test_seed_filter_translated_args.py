"""CPU tier of the ungapped filter for the codon and translated-index lists: exported symbols and header declarations, every refusal
of pmx_seed_ungapped_translated[_device] and pmx_seed_filter_translated[_device] that needs no GPU -- the wrapped sets and fake
pointers of test_seed_filter_args.py, never followed --, the accepted edges with n == 0, and the Python mirror's dispatch by
hits.kind.  Every call with n > 0 below ends before the device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmx_seed_ungapped_translated_device", "pmx_seed_ungapped_translated", "pmx_seed_filter_translated_device", "pmx_seed_filter_translated")
KINDS = (("PMX_SEED_LIST_CODONS", 1), ("PMX_SEED_LIST_REF_FRAMES", 2), ("PMX_SEED_LIST_REF_CODONS", 3))
P = 256                                                                                      # a pointer that is never followed


def _err(pkg):
    return pkg.lib.pmx_last_error().decode()


def test_symbols_and_constants(pkg):
    text = open(os.path.join(ROOT, "include", "parasail_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(pkg.lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    for name, value in KINDS:
        m = re.search(r"#define %s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == value and getattr(pkg, name[4:]) == value
    for name in ("seed_ungapped_translated", "seed_ungapped_translated_device", "seed_filter_translated", "seed_filter_translated_device"):
        assert hasattr(pkg, name), name


@pytest.fixture(scope="module")
def world(pkg):
    class W:
        pass
    w = W()
    w.Q = pkg.SeqSet.wrap_device(P, P, 10, 1000)
    w.R = pkg.SeqSet.wrap_device(P, P, 5, 5000)
    w.dna = pkg.Matrix.create(b"ACGT", 2, -3)
    w.big = pkg.Matrix.create(b"ACGT", 30000, -30000)
    w.pssm = pkg.Matrix.create_pssm("ACGT", [1, -1, 0, 2] * 6, 6)
    w.cfg = lambda m=None: pkg.pmx_config_t(2, 0, 0, 0, 0, 0, (m or w.dna).inner)
    return w


def _shared_refusals(pkg, w, entry):
    """what the four entries refuse about the list, the configuration and the list's kind: entry(**changes) -> rc; the texts are the
    untranslated entries'"""
    for kind in (1, 2, 3):
        assert entry(kind=kind, q=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(kind=kind, r=None) == -1 and "null sequence set" in _err(pkg)
        assert entry(kind=kind, n=-1) == -1 and "negative n" in _err(pkg)
        assert entry(kind=kind, pairs=None) == -1 and "null pairs or records" in _err(pkg)
        assert entry(kind=kind, seeds=None) == -1 and "null seed records" in _err(pkg)
        assert entry(kind=kind, chunk=-1) == -1 and "chunk_pairs must not be negative" in _err(pkg)
        assert entry(kind=kind, cfg=None) == -1 and "null config or matrix" in _err(pkg)
        assert entry(kind=kind, cfg=pkg.pmx_config_t(2, 0, 0, 0, 0, 0, None)) == -1 and "null config or matrix" in _err(pkg)
        assert entry(kind=kind, cfg=w.cfg(w.pssm)) == -1 and "no PSSM" in _err(pkg)
    for bad in (0, 4, -1, 7):
        assert entry(kind=bad) == -1 and "unknown list_kind %d" % bad in _err(pkg)
        assert all(name in _err(pkg) for name, _ in KINDS)


def test_ungapped_refusals_without_gpu(pkg, world):
    w, L = world, pkg.lib

    def dev(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=1, seeds=P, mq=150, mr=400, out=P, cfg=w.cfg(), chunk=0):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_ungapped_translated_device(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, mq, mr, out,
                                                     None, C.byref(o))

    def host(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=1, seeds=P, out=P, cfg=w.cfg(), chunk=0, **unused):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_ungapped_translated(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, out, C.byref(o))

    for entry in (dev, host):
        _shared_refusals(pkg, w, entry)
        assert entry(out=None) == -1 and "null pairs or records" in _err(pkg)
        for kind in (1, 2, 3):
            assert entry(n=0, kind=kind, pairs=None, byte=None, seeds=None, out=None) == 0
    for kind in (1, 2, 3):
        for mq, mr in ((0, 10), (10, 0), (-4, 10)):
            assert dev(kind=kind, mq=mq, mr=mr) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    # max |w| x the cells of the longest diagonal >= 2^31, |w| = 30000: 71583 cells are refused, 71582 fit.  A codon side has one
    # cell per codon of its stream (ceil(max / 3)), and no diagonal is longer than the other side's letters.
    big = w.cfg(w.big)
    assert dev(kind=1, cfg=big, mq=3 * 71583, mr=1 << 20) == -1 and "does not fit int32" in _err(pkg) and "30000 x 71583" in _err(pkg)
    assert dev(kind=1, cfg=big, mq=3 * 71582, mr=1 << 20, n=0) == 0
    assert dev(kind=1, cfg=big, mq=3 * 71583 - 2, mr=1 << 20) == -1 and "30000 x 71583" in _err(pkg)      # ceil
    assert dev(kind=1, cfg=big, mq=1 << 22, mr=71582, n=0) == 0                              # the reference's letters bound it
    assert dev(kind=1, cfg=big, mq=1 << 22, mr=71583) == -1 and "does not fit int32" in _err(pkg)
    assert dev(kind=3, cfg=big, mq=1 << 20, mr=3 * 71583) == -1 and "30000 x 71583" in _err(pkg)
    assert dev(kind=3, cfg=big, mq=1 << 20, mr=3 * 71582, n=0) == 0
    assert dev(kind=3, cfg=big, mq=71583, mr=1 << 22) == -1 and "does not fit int32" in _err(pkg)
    assert dev(kind=3, cfg=big, mq=71582, mr=1 << 22, n=0) == 0
    assert dev(kind=2, cfg=big, mq=71583, mr=71583) == -1 and "30000 x 71583" in _err(pkg)
    assert dev(kind=2, cfg=big, mq=71582, mr=1 << 22, n=0) == 0 and dev(kind=2, cfg=big, mq=1 << 22, mr=71582, n=0) == 0


def test_filter_refusals_without_gpu(pkg, world):
    w, L = world, pkg.lib
    FO = pkg.pmx_seed_filter_opts_t

    def dev(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=3, seeds=P, mq=150, mr=400, cfg=w.cfg(), chunk=0, nq=2, off=P, f=FO(0, 0),
            cap=8, ooff=P, cnt=P):
        o = pkg.pmx_pairs_opts_t(chunk)
        return L.pmx_seed_filter_translated_device(C.byref(cfg) if cfg is not None else None, q, r, n, pairs, byte, kind, None, seeds, mq, mr, nq, off,
                                                   C.byref(f) if f is not None else None, P, P, P, P, P, cap, ooff, cnt, None, C.byref(o))

    _shared_refusals(pkg, w, dev)
    for mq, mr in ((0, 10), (10, 0)):
        assert dev(mq=mq, mr=mr) == -1 and "max_qlen / max_rlen must be positive" in _err(pkg)
    assert dev(cfg=w.cfg(w.big), mq=71583, mr=1 << 22) == -1 and "does not fit int32" in _err(pkg)
    assert dev(f=None) == -1 and "null filter opts" in _err(pkg)
    assert dev(f=FO(0, -1)) == -1 and "top_n -1 is negative" in _err(pkg)
    assert dev(f=FO(-1, 0)) == -1 and "min_score -1 is negative" in _err(pkg)
    for res in ((1, 0), (0, 5)):
        assert dev(f=FO(0, 0, res)) == -1 and "reserved must be 0" in _err(pkg)
    assert dev(nq=-1) == -1 and "negative nq or capacity" in _err(pkg)
    assert dev(cap=-1) == -1 and "negative nq or capacity" in _err(pkg)
    assert dev(off=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(ooff=None) == -1 and "null row offsets" in _err(pkg)
    assert dev(cnt=None) == -1 and "null counts" in _err(pkg)
    assert dev(nq=0) == -1 and "4 candidates in no row" in _err(pkg)
    assert dev(n=1 << 31) == -1 and "beyond 2^31 - 1" in _err(pkg)

    off = np.zeros(4, dtype=np.int64)

    def host(q=w.Q.inner, r=w.R.inner, n=4, pairs=P, byte=P, kind=2, seeds=P, cfg=w.cfg(), chunk=0, f=FO(0, 0), hits=True, passing=None,
             rows=3, row_off=off.ctypes.data, res=True, **unused):
        h = pkg.pmx_seed_hits_t(rows, n, n if passing is None else passing, row_off, pairs, byte, seeds)
        o = pkg.pmx_pairs_opts_t(chunk)
        out = C.POINTER(pkg.pmx_seed_filtered_t)()
        rc = L.pmx_seed_filter_translated(C.byref(cfg) if cfg is not None else None, q, r, C.byref(h) if hits else None, kind, None,
                                          C.byref(f) if f is not None else None, C.byref(o), C.byref(out) if res else None)
        if rc == 0:
            b = out.contents
            assert b.hits.n_rows == rows and b.hits.n_hits == 0 and b.hits.n_passing == 0
            assert [C.cast(b.hits.row_off, C.POINTER(C.c_int64))[x] for x in range(rows + 1)] == [0] * (rows + 1)
            L.pmx_seed_filtered_free(out)
        else:
            assert not out
        return rc

    _shared_refusals(pkg, w, host)
    assert host(res=False) == -1 and "null result pointer" in _err(pkg)
    assert host(hits=False) == -1 and "null hits" in _err(pkg)
    assert host(n=4, passing=9) == -1 and "max_hits cut" in _err(pkg) and "4 of 9" in _err(pkg)
    assert host(rows=-1) == -1 and "negative n_hits or n_rows" in _err(pkg)
    assert host(f=None) == -1 and "null filter opts" in _err(pkg)
    assert host(f=FO(0, -3)) == -1 and "top_n -3 is negative" in _err(pkg)
    assert host(f=FO(-2, 0)) == -1 and "min_score -2 is negative" in _err(pkg)
    assert host(f=FO(0, 0, (0, 1))) == -1 and "reserved must be 0" in _err(pkg)
    assert host(row_off=None) == -1 and "null row offsets" in _err(pkg)
    assert host(rows=0) == -1 and "4 candidates in no row" in _err(pkg)
    for kind in (1, 2, 3):
        for f in (FO(0, 0), FO(40, 3)):
            assert host(n=0, pairs=None, byte=None, seeds=None, kind=kind, f=f) == 0
    assert host(n=0, pairs=None, byte=None, seeds=None, rows=0) == 0


def test_python_mirror_dispatch_by_kind(pkg, world):
    w = world
    S = pkg.SeqSet.wrap_device(P, P, 3, 12)
    empty = pkg.SeqSet.wrap_device(P, P, 0, 0)
    dna = pkg.SeedIndex.build(empty, 12)
    let = pkg.SeedIndex.build(empty, 4, alphabet="aa11")
    tra = pkg.SeedIndex.build(empty, 4, alphabet="aa11", translated="both")
    kinds = [(dna, {}, "strand"), (let, {"frames": "letters"}, "letters"), (let, {"frames": 4}, "frame"), (let, {"frames": "all"}, "frame"),
             (let, {"frames": "codons"}, "codons"), (let, {"frames": "codons-both"}, "codons"), (tra, {"ref_frames": "frames"}, "ref_frames"),
             (tra, {"ref_frames": "codons"}, "ref_codons")]
    for ix, kw, kind in kinds:
        h = pkg.seed_pairs(S, ix, rows=0, **kw)
        assert h.kind == kind, kw
        if kind in ("strand", "letters", "frame"):                                           # refused, and the text names seed_filter
            with pytest.raises(pkg.BatchError, match="kind \"%s\" goes to seed_filter" % kind):
                pkg.seed_filter_translated(S, S, h, w.dna)
        else:                                                                                # an empty list: no GPU work
            f = pkg.seed_filter_translated(S, S, h, w.dna, min_score=10, top_n=2)
            assert isinstance(f, pkg.SeedHits) and f.kind == kind and len(f) == 0 and f.row_off.tolist() == [0]
            assert f.ungapped.dtype == pkg.UNGAPPED_DTYPE and len(f.ungapped) == 0 and f.source.dtype == np.int64 and len(f.source) == 0
            assert (f.frame is not None) == (kind == "ref_frames") and f.seeds.dtype == pkg.SEED_HIT_DTYPE
    h = pkg.seed_pairs(S, dna, rows=0)
    h.kind = None                                                                            # a list of unknown origin is not guessed at
    with pytest.raises(pkg.BatchError, match="goes to seed_filter"):
        pkg.seed_filter_translated(S, S, h, w.dna)
    h = pkg.seed_pairs(S, tra, rows=0, ref_frames="codons")
    with pytest.raises(pkg.BatchError, match="top_n -1 is negative"):
        pkg.seed_filter_translated(S, S, h, w.dna, top_n=-1)
    with pytest.raises(pkg.BatchError, match="min_score -1 is negative"):
        pkg.seed_filter_translated(S, S, h, w.dna, min_score=-1)
    with pytest.raises(pkg.BatchError, match="no PSSM"):
        pkg.seed_filter_translated(S, S, h, w.pssm)
    with pytest.raises(pkg.BatchError, match="a Matrix"):
        pkg.seed_filter_translated(S, S, h, None)
    with pytest.raises(pkg.BatchError, match="64 letters"):                                  # a code that is not 64 letters: the mirror can tell
        pkg.seed_filter_translated(S, S, h, w.dna, code=b"FF")
    h.n_passing = 5
    with pytest.raises(pkg.BatchError, match="max_hits cut"):
        pkg.seed_filter_translated(S, S, h, w.dna)
    none = np.zeros(0, dtype=pkg.PAIR_DTYPE)
    seeds = np.zeros(0, dtype=pkg.SEED_HIT_DTYPE)
    for kind in ("codons", "ref_frames", "ref_codons"):
        assert len(pkg.seed_ungapped_translated(S, S, none, None, seeds, w.dna, kind)) == 0
        assert pkg.seed_ungapped_translated(S, S, none, None, seeds, w.dna, kind, code=b"F" * 64).dtype == pkg.UNGAPPED_DTYPE
    for kind in ("strand", "frame", "letters", 1):
        with pytest.raises(pkg.BatchError, match="\"codons\", \"ref_frames\" or \"ref_codons\""):
            pkg.seed_ungapped_translated(S, S, none, None, seeds, w.dna, kind)
    with pytest.raises(pkg.BatchError, match="seeds and pairs differ"):
        pkg.seed_ungapped_translated(S, S, none, None, np.zeros(2, dtype=pkg.SEED_HIT_DTYPE), w.dna, "codons")
    with pytest.raises(pkg.BatchError, match="64 letters"):
        pkg.seed_ungapped_translated(S, S, none, None, seeds, w.dna, "codons", code=b"F" * 63)
    with pytest.raises(pkg.BatchError, match="max_qlen / max_rlen must be positive"):
        pkg.seed_ungapped_translated_device(S, S, 1, P, None, P, 0, 5, w.dna, P, "ref_codons")
    with pytest.raises(pkg.BatchError, match="top_n -2 is negative"):
        pkg.seed_filter_translated_device(S, S, 1, P, None, P, 5, 5, w.dna, 1, P, None, None, None, None, None, 0, P, P, "ref_frames", top_n=-2)
