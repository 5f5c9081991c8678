"""The CPU model of the reference-side frameshift traceback entries (include/parasail_amd.h, "Frameshift traceback, reference side")
for the tests: tests/swfsc_trace_model.c compiled on first use, the results of a pair list with the bad-pair rule, and what reads a
text back -- its steps cell by cell and its score -- in Python, from the text alone.  UNITS OF THIS SIDE: rows are query letters,
columns are letters of the reference's codon stream = nucleotides of the oriented reference window."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import pairs_ref
import translate_ref

HERE = os.path.dirname(os.path.abspath(__file__))
LETTERS = "MIDNSHP=X/\\"            # op codes 0 .. 10; the query gap is 'I', the codon gap 'D' (include/pmx_conventions.h)
QUERY_GAP, CODON_GAP, SHORT, LONG = "I", "D", "/", "\\"
BAD = list(pairs_ref.BAD_RECORD)
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="swfsc_trace_model"), "swfsc_trace_model.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "swfsc_trace_model.c")], check=True)
        _lib = C.CDLL(so)
        _lib.swfsc_trace_align.restype = C.c_int
        _lib.swfsc_trace_pair.restype = C.c_int
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def text_of(ops):
    return "".join("%d%s" % (int(o) >> 4, LETTERS[int(o) & 15]) for o in ops)


def align(q, T, om, open_, ext, fs):
    """one protein (rows) against one codon stream (columns) -> (record, text, begins, statistics)"""
    qq = np.frombuffer(bytes(q), dtype=np.uint8); t = np.frombuffer(bytes(T), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32); beg = np.zeros(2, dtype=np.int32); st = np.zeros(3, dtype=np.int32)
    ops = np.zeros(len(t) + len(qq) + 1, dtype=np.uint32)
    n = lib().swfsc_trace_align(_p(qq), len(qq), _p(t), len(t), _p(om.scores), _p(om.mapper), om.size, int(open_), int(ext),
                                C.c_longlong(int(fs)), _p(rec), _p(ops), _p(beg), _p(st))
    return rec.tolist(), text_of(ops[:n]), beg.tolist(), st.tolist()


def pair(q, window, mode, om, open_, ext, fs, code=translate_ref.CODE_STD):
    """a protein against a nucleotide reference window on the reference strands of `mode` -> (record, strand, text, begins, statistics)"""
    qq = np.frombuffer(bytes(q), dtype=np.uint8); w = np.frombuffer(bytes(window), dtype=np.uint8)
    cd = np.frombuffer(bytes(code), dtype=np.uint8)
    rec = np.zeros(4, dtype=np.int32); beg = np.zeros(2, dtype=np.int32); st = np.zeros(3, dtype=np.int32)
    strand = np.zeros(1, dtype=np.uint8)
    ops = np.zeros(len(w) + len(qq) + 1, dtype=np.uint32)
    n = lib().swfsc_trace_pair(_p(qq), len(qq), _p(w), len(w), int(mode), _p(cd), _p(om.scores), _p(om.mapper), om.size, int(open_), int(ext),
                               C.c_longlong(int(fs)), _p(rec), _p(strand), _p(ops), _p(beg), _p(st))
    return rec.tolist(), int(strand[0]), text_of(ops[:n]), beg.tolist(), st.tolist()


class Results:
    """records [n, 4], strand [n], texts (list of str), off [n + 1], beg [n, 2], stats [n, 3] of a pair list"""

    def text_bytes(self):
        return "".join(self.texts).encode()


def results(qseqs, rseqs, pairs, mode, om, open_, ext, fs, strands=None, max_qlen=pairs_ref.INT32_MAX, max_rlen=pairs_ref.INT32_MAX,
            code=translate_ref.CODE_STD):
    """what the device entry returns for a pair list: mode for all pairs, or (mode 0) one strand byte per pair; a bad descriptor, a
    query beyond max_qlen, a strand byte above 1, W < 3 and W - 2 > max_rlen give the bad record, strand 0, an empty text, begins
    -1 / -1, zero statistics"""
    n = len(pairs)
    out = Results()
    out.records = np.zeros((n, 4), dtype=np.int32); out.strand = np.zeros(n, dtype=np.uint8)
    out.beg = np.full((n, 2), -1, dtype=np.int32); out.stats = np.zeros((n, 3), dtype=np.int32)
    out.texts = []
    for k, d in enumerate(pairs):
        q = pairs_ref.resolve_side(qseqs, d["q"], d["q_beg"], d["q_len"], max_qlen)
        r = pairs_ref.resolve_side(rseqs, d["r"], d["r_beg"], d["r_len"])
        m = mode if strands is None else int(strands[k])
        if q is None or r is None or len(r) < 3 or len(r) - 2 > max_rlen or (strands is not None and m > 1):
            out.records[k] = BAD
            out.texts.append("")
            continue
        out.records[k], out.strand[k], text, out.beg[k], out.stats[k] = pair(q, r, m, om, open_, ext, fs, code)
        out.texts.append(text)
    out.off = np.concatenate([[0], np.cumsum([len(t) for t in out.texts])]).astype(np.int64)
    return out


def parse(text):
    """-> [(count, op)]; raises on anything that is not <count><op> over the eleven letters"""
    runs = re.findall(r"(\d+)([MIDNSHP=X/\\])", text)
    assert "".join(c + o for c, o in runs) == text, text
    return [(int(c), o) for c, o in runs]


def steps(text, beg):
    """the path of a text from its begin cell, one entry per column op: (op, source row, row, column, how).  A match column's source
    row is the row of the cell before it on the path (None for the first); a frameshift op belongs to the match column behind it
    and is reported with it as '/' or '\\' in place of the in-frame step's '3'.  A match column and a query gap go from row - 1 to
    row; a codon gap stays in its row and goes from column - 3 to column."""
    out = []
    i, j = None, None
    pending = 3
    for count, op in parse(text):
        for _ in range(count):
            if op in "=X":
                if i is None:
                    assert pending == 3
                    i, j = beg
                    out.append((op, None, i, j, "start"))
                else:
                    out.append((op, i, i + 1, j + pending, {3: "3", 2: SHORT, 4: LONG}[pending]))
                    i, j = i + 1, j + pending
                pending = 3
            elif op == SHORT or op == LONG:
                assert pending == 3 and count == 1 and i is not None
                pending = 2 if op == SHORT else 4
            elif op == QUERY_GAP:
                assert pending == 3 and i is not None
                out.append((op, i, i + 1, j, QUERY_GAP))
                i += 1
            elif op == CODON_GAP:
                assert pending == 3 and i is not None
                out.append((op, i, i, j + 3, CODON_GAP))
                j += 3
            else:
                raise AssertionError(op)
    assert pending == 3
    return out


def rescore(text, beg, q, T, score, open_, ext, fs):
    """(score, end_query, end_ref) of a text read from `beg` over the protein q and the codon stream T, from the text alone: matrix
    scores score(query letter, stream letter), open / ext per gap run of one kind, fs per frameshift op.  Checks '=' / 'X' against
    the letters (equality is decided by score.same where the matrix maps several letters to one index)."""
    same = getattr(score, "same", lambda a, b: a == b)
    total, last, i, j = 0, None, None, None
    for op, _, row, col, how in steps(text, beg):
        if op in "=X":
            assert (op == "=") == bool(same(q[row], T[col])), (text, row, col)
            total += score(q[row], T[col]) - (fs if how in (SHORT, LONG) else 0)
            last = "M"
        else:
            total -= ext if last == op else open_
            last = op
        i, j = row, col
    if i is None:
        return 0, beg[0] - 1, beg[1] - 1
    return total, i, j + 2


def counts(text):
    """match columns, query gaps, codon gaps, '/' and '\\' of a text"""
    c = {"m": 0, QUERY_GAP: 0, CODON_GAP: 0, SHORT: 0, LONG: 0}
    for count, op in parse(text):
        c["m" if op in "=X" else op] += count
    return c
