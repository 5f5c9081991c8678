"""Plain Python restatement of the strands of the sequence-set batches (include/parasail_amd.h): the complement table, the
reverse complement of a window, and descriptors + strand bytes resolved to byte strings.  Written from the specification; it does not
read the library's table."""
import pairs_ref

INT32_MAX = pairs_ref.INT32_MAX
BAD_BEGIN = (-1, -1)


def complement_table():
    """256 bytes: "ACGTUMRWSYKVHDBN" -> "TGCAAKYWSRMBDHVN", lower case the same way to lower case, every other byte itself."""
    t = bytearray(range(256))
    for a, b in zip(b"ACGTUMRWSYKVHDBN", b"TGCAAKYWSRMBDHVN"):
        t[a] = b
        t[a + 32] = b + 32
    return bytes(t)


COMP = complement_table()


def revcomp(window):
    """w'[x] = comp[w[L - 1 - x]]"""
    return bytes(window[::-1]).translate(COMP)


def resolve(qseqs, rseqs, pairs, strand=None, max_qlen=INT32_MAX, max_rlen=INT32_MAX):
    """[(query bytes, reference bytes) or None for a bad pair]: pairs_ref.resolve with the strand applied to the query window; a
    strand byte other than 0 or 1 makes the pair bad."""
    out = pairs_ref.resolve(qseqs, rseqs, pairs, max_qlen, max_rlen)
    if strand is None:
        return out
    assert len(strand) == len(pairs)
    for k, s in enumerate(strand):
        if out[k] is None:
            continue
        if int(s) > 1:
            out[k] = None
        elif int(s) == 1:
            out[k] = (revcomp(out[k][0]), out[k][1])
    return out
