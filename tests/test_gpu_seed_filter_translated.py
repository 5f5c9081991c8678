"""The ungapped diagonal filter over the codon and translated-index lists (`-m gpu`): pmx_seed_ungapped_translated[_device] and
pmx_seed_filter_translated[_device] against the model tests/seed_filter_translated_ref.py.  Every comparison is exact, byte for byte;
every output buffer starts as a sentinel and is checked behind `capacity`.

The lists are those of tests/seed_filter_translated_lists.py (what they reach is asserted on the model, on the CPU tier): cells per
diagonal 1 .. 9, 63 .. 65, 127 .. 129, 255 .. 257, 398 .. 400 with W = 3 c + 2 + {0, 1, 2} on a codon side, spans 1 .. 5, 8, 9, 15 .. 17
and 300 nucleotide diagonals, both strands of the strided side, windows clipped on either side (on strand 1 with N != r_beg + r_len),
diagonals with no cell, N / stop / lower case in the streams, ties, and every kind of bad candidate between good neighbours."""
import numpy as np
import pytest

import seed_filter_translated_lists as lists
import seed_filter_translated_ref as ref
import seed_translated_ref

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0xA5
KINDS = ("codons", "ref_codons", "ref_frames")
BUILD = {"codons": lists.codons_list, "ref_codons": lists.ref_codons_list, "ref_frames": lists.ref_frames_list}
KERNEL = {"codons": "pmx_ungapped_kernel<codons>", "ref_codons": "pmx_ungapped_kernel<ref_codons>", "ref_frames": "pmx_ungapped_kernel<ref_frames>"}
OPEN, EXT, SHIFT = 11, 1, 15


def _dev():
    import torch
    return torch.device("cuda", 0)


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=_dev())


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def _assert_same(got, want):
    diff = np.nonzero((got.view(np.int32).reshape(-1, 4) != want.view(np.int32).reshape(-1, 4)).any(axis=1))[0]
    assert len(diff) == 0, "candidate %d: got %s, want %s (%d differ)" % (diff[0], tuple(got[diff[0]]), tuple(want[diff[0]]), len(diff))


@pytest.fixture(scope="module")
def b62(pkg):
    m = pkg.Matrix.from_name("blosum62")
    assert m.size <= 32                                                                      # the table staged as bytes in LDS
    return m, m.to_numpy(), m.mapper()


@pytest.fixture(scope="module")
def built():
    """the three hand-built lists, computed once, never changed"""
    return {kind: BUILD[kind]() for kind in KINDS}


@pytest.fixture(scope="module")
def wants(built, b62):
    """the model's records of each list under the list's own maxima"""
    _, scores, mapper = b62
    return {kind: ref.ungapped(L.qs, L.refs, L.pairs, L.byte, L.seeds, scores, mapper, kind, max_qlen=L.max_qlen, max_rlen=L.max_rlen)
            for kind, L in built.items()}


def _ungapped_device(pkg, Q, R, pairs, byte, seeds, mq, mr, matrix, kind, code=None, chunk_pairs=0):
    import torch
    n = len(pairs)
    out = _full((n + 3, 4), SENTINEL, torch.int32)
    dp, ds = _up(pairs), _up(seeds)
    db = _up(byte) if byte is not None else None
    pkg.seed_ungapped_translated_device(Q, R, n, dp.data_ptr(), db.data_ptr() if db is not None else None, ds.data_ptr(), mq, mr, matrix,
                                        out.data_ptr(), kind, code=code, stream=_stream(), chunk_pairs=chunk_pairs)
    _sync()
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    return got[:n].reshape(-1).view(ref.UNGAPPED_DTYPE)


@pytest.mark.parametrize("chunk_pairs", [0, 1, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_records_equal_the_model_under_any_chunking(pkg, built, wants, b62, kind, chunk_pairs):
    L, m = built[kind], b62[0]
    Q, R = pkg.SeqSet.new(L.qs), pkg.SeqSet.new(L.refs)
    got = _ungapped_device(pkg, Q, R, L.pairs, L.byte, L.seeds, L.max_qlen, L.max_rlen, m, kind, chunk_pairs=chunk_pairs)
    _assert_same(got, wants[kind])
    if chunk_pairs == 0:
        assert pkg.lib.pmx_last_kernel().decode() == KERNEL[kind]
        again = _ungapped_device(pkg, Q, R, L.pairs, L.byte, L.seeds, L.max_qlen, L.max_rlen, m, kind)
        assert again.tobytes() == got.tobytes()                                              # determinism: a second run, the same bytes
        # the host entry finds the maxima itself: the candidates that only the list's maxima made bad are good there
        host = ref.ungapped(L.qs, L.refs, L.pairs, L.byte, L.seeds, b62[1], b62[2], kind)
        assert (host["score"] == -1).sum() < (wants[kind]["score"] == -1).sum()
        _assert_same(pkg.seed_ungapped_translated(Q, R, L.pairs, L.byte, L.seeds, m, kind), host)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_table_custom_code_and_no_bytes(pkg, built, kind):
    """a 24-letter matrix with scores outside a byte (the int16 table through L1), a custom genetic code, and d_byte NULL (all 0)"""
    L = built[kind]
    wide = pkg.Matrix.create(b"ARNDCQEGHILKMFPSTWYVBZX", 300, -200)
    assert wide.size == 24
    Q, R = pkg.SeqSet.new(L.qs), pkg.SeqSet.new(L.refs)
    keep = np.arange(0, len(L.pairs), 3)
    p, b, s = L.pairs[keep], L.byte[keep], L.seeds[keep]
    want = ref.ungapped(L.qs, L.refs, p, b, s, wide.to_numpy(), wide.mapper(), kind, code=lists.CUSTOM_CODE, max_qlen=L.max_qlen, max_rlen=L.max_rlen)
    std = ref.ungapped(L.qs, L.refs, p, b, s, wide.to_numpy(), wide.mapper(), kind, max_qlen=L.max_qlen, max_rlen=L.max_rlen)
    assert want["score"].max() > 30000 and (want["score"] != std["score"]).sum() > 10         # the code matters
    _assert_same(_ungapped_device(pkg, Q, R, p, b, s, L.max_qlen, L.max_rlen, wide, kind, code=lists.CUSTOM_CODE, chunk_pairs=13), want)
    fwd = np.nonzero(L.byte == 0)[0][::2]
    want = ref.ungapped(L.qs, L.refs, L.pairs[fwd], None, L.seeds[fwd], wide.to_numpy(), wide.mapper(), kind, max_qlen=L.max_qlen, max_rlen=L.max_rlen)
    assert (want["score"] > 0).sum() > 40
    _assert_same(_ungapped_device(pkg, Q, R, L.pairs[fwd], None, L.seeds[fwd], L.max_qlen, L.max_rlen, wide, kind), want)


# ---- the device filter entry: capacity, sentinels, empty lists, determinism, ties ---------------------------------------------------------
class _Hits:
    """what the mirror's seed_filter_translated reads of a SeedHits, from a model list"""

    def __init__(self, kind, h, n_rows):
        self.kind, self.n_rows, self.n_hits, self.n_passing = kind, n_rows, len(h["pairs"]), len(h["pairs"])
        self.row_off, self.pairs, self.seeds = h["row_off"], h["pairs"], h["seeds"]
        self.strand, self.frame = (np.zeros(len(h["byte"]), dtype=np.uint8), h["byte"]) if kind == "ref_frames" else (h["byte"], None)


def _filter_device(pkg, Q, R, kind, h, nq, matrix, mq, mr, capacity, skip=(), **kw):
    import torch
    n = len(h["pairs"])
    slots = capacity + 3
    op = _full((slots * 32,), FILL, torch.uint8)
    ob = _full((slots,), FILL, torch.uint8)
    os_ = _full((slots, 4), SENTINEL, torch.int32)
    ou = _full((slots, 4), SENTINEL, torch.int32)
    osrc = _full((slots,), SENTINEL, torch.int64)
    off = _full((nq + 1 + 2,), SENTINEL, torch.int64)
    cnt = _full((2 + 2,), SENTINEL, torch.int64)
    dp, db, ds, dro = _up(h["pairs"]), _up(h["byte"]), _up(h["seeds"]), _up(h["row_off"])
    ptr = lambda name, t: None if name in skip else t.data_ptr()
    pkg.seed_filter_translated_device(Q, R, n, dp.data_ptr() if n else None, db.data_ptr() if n else None, ds.data_ptr() if n else None, mq, mr, matrix,
                                      nq, dro.data_ptr(), ptr("pairs", op), ptr("byte", ob), ptr("seeds", os_), ptr("ungapped", ou), ptr("source", osrc),
                                      capacity, off.data_ptr(), cnt.data_ptr(), kind, stream=_stream(), **kw)
    _sync()
    return {"pairs": op.cpu().numpy().view(ref.pairs_ref.PAIR_DTYPE), "byte": ob.cpu().numpy(), "seeds": os_.cpu().numpy().reshape(-1).view(ref.SEED_HIT_DTYPE),
            "ungapped": ou.cpu().numpy().reshape(-1).view(ref.UNGAPPED_DTYPE), "source": osrc.cpu().numpy(), "row_off": off.cpu().numpy(),
            "counts": cnt.cpu().numpy()}


def _same_device(g, want, capacity, nq, skip=()):
    kept = want["counts"][0]
    w = min(kept, capacity)
    assert g["row_off"][:nq + 1].tolist() == want["row_off"].tolist() and (g["row_off"][nq + 1:] == SENTINEL).all()
    assert g["counts"][:2].tolist() == [kept, w] and (g["counts"][2:] == SENTINEL).all()
    for name, fill in (("pairs", FILL), ("byte", FILL), ("seeds", SENTINEL), ("ungapped", SENTINEL), ("source", SENTINEL)):
        a = g[name]
        raw = a.view(np.uint8 if fill == FILL else np.int64 if name == "source" else np.int32)
        per = len(raw) // len(a)
        if name in skip:
            assert (raw == fill).all(), name
            continue
        assert a[:w].tobytes() == np.ascontiguousarray(want[name][:w]).tobytes(), name
        assert (raw[w * per:] == fill).all(), name                                           # behind the written positions: untouched


def _with_records(kind, qs, rs, planted, hits, b62):
    """a world, and the model's records of its list: computed once, shared by the tests, never changed"""
    return qs, rs, planted, hits, ref.ungapped(qs, rs, hits["pairs"], hits["byte"], hits["seeds"], b62[1], b62[2], kind)


@pytest.fixture(scope="module")
def codon_world(b62):
    prots, reads, planted, hits = lists.codon_world()
    return _with_records("codons", reads, prots, planted, hits, b62)


@pytest.fixture(scope="module")
def tblastn_cut(b62):
    prots, cut, planted = lists.tblastn_world(cut=True)
    return _with_records("ref_codons", prots, cut, planted, lists.tblastn_hits(prots, cut, seed_translated_ref.REF_CODONS), b62)


@pytest.fixture(scope="module")
def tblastn_whole(b62):
    prots, whole, planted = lists.tblastn_world(cut=False)
    return _with_records("ref_frames", prots, whole, planted, lists.tblastn_hits(prots, whole, seed_translated_ref.REF_FRAMES), b62)


def test_device_entry_capacity_sentinels_and_determinism(pkg, codon_world, b62):
    reads, prots, planted, hits, ung = codon_world
    m, scores, mapper = b62
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    nq, mq, mr = len(reads), 150, 110                                                        # (no window is longer: the records are `ung`)
    per_row = np.diff(hits["row_off"])
    assert (per_row == 0).sum() >= 2 and (per_row >= 2).sum() > 10                           # empty rows, rows with several candidates
    model = lambda **kw: ref.filter_hits(reads, prots, hits["row_off"], hits["pairs"], hits["byte"], hits["seeds"], scores, mapper, "codons",
                                         ung=ung, **kw)
    for min_score, top_n in ((0, 0), (30, 2)):
        kept = model(min_score=min_score, top_n=top_n)["counts"][0]
        assert kept > 20
        runs = []
        for cap, chunk in ((kept + 2, 0), (kept, 7), (kept // 2, 0), (1, 0), (0, 0), (kept + 2, 1 if top_n else 0)):
            want = model(min_score=min_score, top_n=top_n, capacity=cap)
            g = _filter_device(pkg, Q, R, "codons", hits, nq, m, mq, mr, cap, min_score=min_score, top_n=top_n, chunk_pairs=chunk)
            _same_device(g, want, cap, nq)
            if cap == kept + 2:
                runs.append(b"".join(g[k].tobytes() for k in sorted(g)))
        assert runs[0] == runs[1]                                                            # run to run, and under another chunking
    skip = ("pairs", "seeds", "source")                                                      # every output column is optional
    _same_device(_filter_device(pkg, Q, R, "codons", hits, nq, m, mq, mr, 5, top_n=1, skip=skip), model(top_n=1, capacity=5), 5, nq, skip)
    for n_rows in (0, 5):                                                                    # the empty list
        e = {"pairs": hits["pairs"][:0], "byte": hits["byte"][:0], "seeds": hits["seeds"][:0], "row_off": np.zeros(n_rows + 1, dtype=np.int64)}
        want = dict(e, counts=[0, 0], ungapped=np.zeros(0, dtype=ref.UNGAPPED_DTYPE), source=np.zeros(0, dtype=np.int64))
        _same_device(_filter_device(pkg, Q, R, "codons", e, n_rows, m, mq, mr, 4, top_n=2), want, 4, n_rows)


def test_top_n_ties_keep_the_earlier_position(pkg, b62):
    """a protein whose gene lies three times in one contig and once, with one letter changed, in another: three equal candidates and
    one lesser in a row, an empty row, and a row of two; top_n 1 .. 4 through the host entry and the model"""
    m, scores, mapper = b62
    rng = np.random.default_rng(9600)
    prot = lists.random_protein(rng, 30)
    gene = lists.back_translate(prot, rng)
    other = lists.back_translate(prot[:10] + (b"W" if prot[10:11] != b"W" else b"A") + prot[11:], rng)
    gap = b"TAATAGTGA"
    contigs = [b"AC" + gene + gap + b"G" + gene + gap + gene + b"TAC", b"GGA" + other + b"TAA"]
    at = [2, 2 + 90 + 10, 2 + 90 + 10 + 90 + 9]
    qs = [prot, b"MKW", prot[:10]]
    rows, sd = [], []
    for a in at:
        rows.append((0, 0, 0, -1, a, 92))
        sd.append((a, a, 0))
    rows.append((0, 1, 0, -1, 0, len(contigs[1])))
    sd.append((3, 3, 0))
    rows += [(2, 0, 0, -1, 0, len(contigs[0])), (2, 1, 0, -1, 0, len(contigs[1]))]
    sd += [(0, 250, 0), (3, 3, 0)]
    h = {"row_off": np.array([0, 4, 4, 6], dtype=np.int64), "pairs": ref.pairs_ref.pairs_array(rows), "byte": np.zeros(6, dtype=np.uint8),
         "seeds": lists.seeds_array(sd)}
    Q, R = pkg.SeqSet.new(qs), pkg.SeqSet.new(contigs)
    hits = _Hits("ref_codons", h, 3)
    full = pkg.seed_filter_translated(Q, R, hits, m)
    sc = full.ungapped["score"].tolist()
    assert sc[0] == sc[1] == sc[2] > sc[3] > 100 and sc[4] == sc[5] > 30 and full.source.tolist() == [0, 1, 2, 3, 4, 5]
    for top_n, kept in ((1, [0, 4]), (2, [0, 1, 4, 5]), (3, [0, 1, 2, 4, 5]), (4, [0, 1, 2, 3, 4, 5])):
        f = pkg.seed_filter_translated(Q, R, hits, m, top_n=top_n)
        want = ref.filter_hits(qs, contigs, h["row_off"], h["pairs"], h["byte"], h["seeds"], scores, mapper, "ref_codons", top_n=top_n)
        assert f.source.tolist() == kept == want["source"].tolist() and f.row_off.tolist() == want["row_off"].tolist()
        assert f.ungapped.tobytes() == want["ungapped"].tobytes() and f.kind == "ref_codons" and f.frame is None


# ---- the three roads end to end --------------------------------------------------------------------------------------------------------
def _same_list(hits, want, frame):
    byte = hits.frame if frame else hits.strand
    assert hits.row_off.tobytes() == want["row_off"].tobytes() and hits.pairs.tobytes() == want["pairs"].tobytes()
    assert byte.tobytes() == want["byte"].tobytes() and hits.seeds.tobytes() == want["seeds"].tobytes()


def _same_hits(f, want, kind, n_rows):
    assert f.kind == kind and f.n_rows == n_rows and f.n_hits == len(f) == want["counts"][0] == f.n_passing
    assert f.row_off.tobytes() == want["row_off"].tobytes()
    assert f.pairs.tobytes() == want["pairs"].tobytes() and f.seeds.tobytes() == want["seeds"].tobytes()
    assert f.ungapped.tobytes() == want["ungapped"].tobytes() and f.source.tobytes() == want["source"].tobytes()
    if kind == "ref_frames":
        assert f.frame.tobytes() == want["byte"].tobytes() and not f.strand.any()
    else:
        assert f.frame is None and f.strand.tobytes() == want["byte"].tobytes()


def _aligner(pkg, m):
    return pkg.Aligner.new().local().matrix(m).gap_open(OPEN).gap_extend(EXT).build()


def test_codon_road_end_to_end(pkg, codon_world, b62):
    reads, prots, planted, model_hits, ung = codon_world
    m, scores, mapper = b62
    want, mine = lists.planted_survivors("codons", reads, prots, model_hits, planted, scores, mapper, ung)
    Q, R = pkg.SeqSet.new(reads), pkg.SeqSet.new(prots)
    ix = pkg.SeedIndex.build(R, lists.K_AA, alphabet="aa11", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=12, pad=8, max_occ=64, frames="codons-both")
    assert hits.kind == "codons"
    _same_list(hits, model_hits, False)
    f = pkg.seed_filter_translated(Q, R, hits, m, top_n=1)
    _same_hits(f, want, "codons", len(reads))
    assert pkg.lib.pmx_last_kernel().decode() == KERNEL["codons"]
    assert all(f.source[int(f.row_off[q])] == x for q, x in mine.items())                   # the planted candidate is the survivor
    _same_hits(pkg.seed_filter_translated(Q, R, hits, m, min_score=35, top_n=2, chunk_pairs=37),
               ref.filter_hits(reads, prots, model_hits["row_off"], model_hits["pairs"], model_hits["byte"], model_hits["seeds"], scores, mapper, "codons",
                               min_score=35, top_n=2, ung=ung), "codons", len(reads))
    al = _aligner(pkg, m)
    rec, strand = al.align_pairs(Q, R, f.pairs, frameshift=SHIFT, strand=f.strand)
    rec_all, _ = al.align_pairs(Q, R, hits.pairs, frameshift=SHIFT, strand=hits.strand)
    assert 0 < len(f) < len(hits) and rec.tobytes() == rec_all[f.source].tobytes() and strand.tobytes() == f.strand.tobytes()
    assert (rec["flags"] == 0).all() and (rec["score"] >= f.ungapped["score"]).all() and (rec["score"] > f.ungapped["score"]).sum() > 100


def test_ref_frames_road_end_to_end(pkg, tblastn_whole, b62):
    prots, whole, planted, model_hits, ung = tblastn_whole
    m, scores, mapper = b62
    want, mine = lists.planted_survivors("ref_frames", prots, whole, model_hits, planted, scores, mapper, ung)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(whole)
    ix = pkg.SeedIndex.build(R, lists.K_AA, alphabet="aa11", translated="both", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=4, pad=8, max_occ=64, ref_frames="frames")
    assert hits.kind == "ref_frames"
    _same_list(hits, model_hits, True)
    f = pkg.seed_filter_translated(Q, R, hits, m, top_n=1)
    _same_hits(f, want, "ref_frames", len(prots))
    assert pkg.lib.pmx_last_kernel().decode() == KERNEL["ref_frames"]
    assert all(f.source[int(f.row_off[q])] == x for q, x in mine.items())
    assert (f.seeds["reserved"] == hits.seeds["reserved"][f.source]).all() and set(f.seeds["reserved"].tolist()) == set(range(6))
    al = _aligner(pkg, m)
    rec, frames = al.align_pairs(Q, R, f.pairs, ref_frame=f.frame)
    rec_all, _ = al.align_pairs(Q, R, hits.pairs, ref_frame=hits.frame)
    assert 0 < len(f) < len(hits) and rec.tobytes() == rec_all[f.source].tobytes() and frames.tobytes() == f.frame.tobytes()
    assert (rec["flags"] == 0).all() and (rec["score"] >= f.ungapped["score"]).all()


def test_ref_codons_road_end_to_end(pkg, tblastn_cut, b62):
    prots, cut, planted, model_hits, ung = tblastn_cut
    m, scores, mapper = b62
    want, mine = lists.planted_survivors("ref_codons", prots, cut, model_hits, planted, scores, mapper, ung)
    Q, R = pkg.SeqSet.new(prots), pkg.SeqSet.new(cut)
    ix = pkg.SeedIndex.build(R, lists.K_AA, alphabet="aa11", translated="both", stream=_stream())
    hits = pkg.seed_pairs(Q, ix, min_seeds=2, band=12, pad=24, max_occ=64, ref_frames="codons")
    assert hits.kind == "ref_codons"
    _same_list(hits, model_hits, False)
    f = pkg.seed_filter_translated(Q, R, hits, m, top_n=1)
    _same_hits(f, want, "ref_codons", len(prots))
    assert pkg.lib.pmx_last_kernel().decode() == KERNEL["ref_codons"]
    assert all(f.source[int(f.row_off[q])] == x for q, x in mine.items())
    al = _aligner(pkg, m)
    rec, strand = al.align_pairs(Q, R, f.pairs, ref_frameshift=SHIFT, ref_strand=f.strand)
    rec_all, _ = al.align_pairs(Q, R, hits.pairs, ref_frameshift=SHIFT, ref_strand=hits.strand)
    rec2, cigars, begins, strand2 = al.align_pairs_frameshift_ref_cigar(Q, R, f.pairs, SHIFT, ref_strand=f.strand)
    assert 0 < len(f) < len(hits) and rec.tobytes() == rec_all[f.source].tobytes() == rec2.tobytes()
    assert strand.tobytes() == strand2.tobytes() == f.strand.tobytes() and (rec["flags"] == 0).all()
    assert (rec["score"] >= f.ungapped["score"]).all() and (rec["score"] > f.ungapped["score"]).sum() > 100
    assert sum("/" in c or "\\" in c for c in cigars) > 100                                  # the survivors' paths cross the deleted nucleotide
