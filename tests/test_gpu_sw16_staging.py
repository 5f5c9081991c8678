"""Per-wave setup of the perm-table local kernel (pmx_sw16.hip, VAR 6): sequences staged by aligned dwords, selectors taken
straight from the staged query letters, wildcards noted by the staging lane, one sweep loop for both parities of the step
count, and the retry launch whose workgroups loop over the device-side list.  Everything runs through the C ABI
(pmx_align_batch_device / pmx_align_profile_batch_device) and every record is compared with the CPU oracle exactly: score,
end_query, end_ref, flags (0: a pair handed back for a wildcard is redone before the call returns).

Batches are 4096 pairs, the smallest the perm-table form takes.  Matrix create("ACGT", 2, -3), gaps 5 / 2."""
import numpy as np
import pytest

from util import DNA, random_seqs

pytestmark = pytest.mark.gpu

N = 4096
RLENS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 149, 150)
QLENS = (1, 3, 4, 5, 19, 20, 133, 149, 150, 151, 152)
GUARD = 8


@pytest.fixture(scope="module")
def env(pkg, orc):
    import torch
    return {"pkg": pkg, "orc": orc, "torch": torch, "dev": torch.device("cuda", 0),
            "pm": pkg.Matrix.create(b"ACGT", 2, -3), "om": orc.Matrix.create("ACGT", 2, -3)}


def _seqs_of(rng, lens):
    return [DNA[rng.integers(0, 4, size=int(l))].tobytes() for l in lens]


def _guarded(env, buf, shift, guard):
    """device copy of `buf` at an interior pointer: GUARD guard bytes, `shift` more, the batch, GUARD guard bytes"""
    host = np.full(len(buf) + 2 * GUARD + shift, ord(guard), dtype=np.uint8)
    host[GUARD + shift:GUARD + shift + len(buf)] = buf
    t = env["torch"].from_numpy(host).to(env["dev"])
    return t, t.data_ptr() + GUARD + shift


def _run_pairs(env, qs, rs, shift=0, guard="A", want=0):
    """records [n, 4] of pmx_align_batch_device and the kernel's name"""
    pkg, torch, dev = env["pkg"], env["torch"], env["dev"]
    qb, qo = pkg.pack(qs); rb, ro = pkg.pack(rs)
    n = len(qs)
    tq, pq = _guarded(env, qb, shift, guard)
    tr, pr = _guarded(env, rb, (shift + 1) & 3, guard)           # the two buffers at different residues
    dqo, dro = torch.from_numpy(qo).to(dev), torch.from_numpy(ro).to(dev)
    out = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 16, want, env["pm"].inner)
    pkg.align_batch_device(cfg, n, pq, dqo.data_ptr(), pr, dro.data_ptr(), int(np.diff(qo).max()), int(np.diff(ro).max()),
                           out.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), pkg.lib.pmx_last_kernel().decode()


def _oracle(env, qs, rs):
    orc = env["orc"]
    qb, qo = orc.pack(qs); rb, ro = orc.pack(rs)
    return orc.align_batch(orc.SW, qb, qo, rb, ro, 5, 2, env["om"])


def _check(got, want, what=""):
    bad = np.nonzero((got[:, :3] != want[:, :3]).any(axis=1) | (got[:, 3] != 0))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def test_staging_every_alignment_and_guard_bytes(env):
    """Lengths 1..150 on both sides: qoff / roff take every residue mod 4.  The batch sits at interior pointers +0..+3 of an
    allocation with 8 guard bytes on both sides; guards of A and of T give the same records: no byte outside the batch
    reaches a result."""
    rng = np.random.default_rng(7101)
    qs, rs = random_seqs(rng, N, 1, 150), random_seqs(rng, N, 1, 150)
    want = _oracle(env, qs, rs)
    for shift in range(4):
        a, name = _run_pairs(env, qs, rs, shift, "A")
        assert "permtable" in name, name
        t, _ = _run_pairs(env, qs, rs, shift, "T")
        assert (a == t).all(), shift
        _check(a, want, shift)


def test_staging_trip_boundaries_and_step_parity(env):
    """Reference lengths around the staging trips (and both parities of the step count, which follows the longest reference)
    and query lengths around the lanes' row dwords: mixed inside every wave, then one length per batch on either side."""
    rng = np.random.default_rng(7102)
    batches = [(rng.choice(QLENS, size=N), rng.choice(RLENS, size=N))]
    batches += [(rng.choice(QLENS, size=N), np.full(N, rl)) for rl in RLENS]
    batches += [(np.full(N, ql), rng.choice(RLENS, size=N)) for ql in QLENS]
    seqs = [(_seqs_of(rng, ql), _seqs_of(rng, rl)) for ql, rl in batches]
    want = _oracle(env, [q for qs, _ in seqs for q in qs], [r for _, rs in seqs for r in rs])    # one oracle call for all
    for k, (qs, rs) in enumerate(seqs):
        got, name = _run_pairs(env, qs, rs, k & 3)
        assert "permtable" in name, (k, name)
        _check(got, want[k * N:(k + 1) * N], k)


def test_staging_last_wave_with_clamped_slots(env):
    rng = np.random.default_rng(7103)
    n = 4099                                    # not a multiple of 16: the last wave repeats the last pair in its spare slots
    qs, rs = random_seqs(rng, n, 100, 150), random_seqs(rng, n, 100, 150)
    got, name = _run_pairs(env, qs, rs, 1)
    assert "permtable" in name, name
    _check(got, _oracle(env, qs, rs))


def _with(seq, at, byte):
    s = bytearray(seq)
    s[at % len(s)] = byte
    return bytes(s)


@pytest.mark.parametrize("case", ["none", "one_pair", "one_per_wave_every_slot", "references_only", "unknown_bytes"])
def test_staging_wildcards(env, case):
    """A query wildcard is seen once, by the lane that stages the letter, and sends exactly that pair to the retry list; the
    records equal the oracle's whatever the path."""
    rng = np.random.default_rng(7104)
    qs, rs = random_seqs(rng, N, 1, 150), random_seqs(rng, N, 1, 150)
    if case == "one_pair":
        qs[1234] = _with(qs[1234], 77, ord("N"))
    elif case == "one_per_wave_every_slot":
        for w in range(N // 16):                # wave w: the pair in slot position w % 16, the letter at a varying row
            k = 16 * w + w % 16
            qs[k] = _with(qs[k], 7 * w, ord("N"))
    elif case == "references_only":
        rs = [_with(r, 3 * k, ord("N")) for k, r in enumerate(rs)]
    elif case == "unknown_bytes":
        odd = (ord("#"), 0xFF, 0x80, ord("n"), ord("x"), 1)
        qs = [_with(q, 5 * k, odd[k % 6]) if k % 3 == 0 else q for k, q in enumerate(qs)]
        rs = [_with(r, 11 * k, odd[(k + 1) % 6]) if k % 4 == 0 else r for k, r in enumerate(rs)]
    got, name = _run_pairs(env, qs, rs, 2)
    assert "permtable" in name, name
    _check(got, _oracle(env, qs, rs), case)


@pytest.mark.parametrize("n,lo,hi", [(8192, 1, 150), (3 * 1024 * 16 + 40, 1, 24)])
def test_staging_every_pair_retried(env, n, lo, hi):
    """A wildcard in every query: the whole batch comes back through the retry launch.  Its workgroups (at most
    PMX_SW16_RETRY_BLOCKS = 1024, 16 pairs each) loop over the list: 8192 pairs are 512 workgroups, one trip each; the second
    batch (short pairs, to keep it quick) is just over three trips per workgroup."""
    rng = np.random.default_rng(7105 + n)
    qs, rs = random_seqs(rng, n, lo, hi), random_seqs(rng, n, lo, hi)
    qs = [_with(q, 13 * k, ord("N")) for k, q in enumerate(qs)]
    got, name = _run_pairs(env, qs, rs, 3)
    assert "permtable" in name, name
    _check(got, _oracle(env, qs, rs), n)


@pytest.mark.parametrize("sorted_", [False, True])
def test_staging_shared_query(env, sorted_):
    """One 1000-letter query against 4096 references of 1..200 letters: pmx_sw16_kernel<64,16,6>, in input order and in
    length-sorted order (the `perm` road)."""
    pkg, torch, dev = env["pkg"], env["torch"], env["dev"]
    rng = np.random.default_rng(7106)
    q = random_seqs(rng, 1, 1000, 1000)[0]
    rs = random_seqs(rng, N, 1, 200)
    rb, ro = pkg.pack(rs)
    tr, pr = _guarded(env, rb, 3, "G")
    dro = torch.from_numpy(ro).to(dev)
    out = torch.full((N, 4), -7, dtype=torch.int32, device=dev)
    prof = pkg.Profile.new(q, False, env["pm"])
    cfg = pkg.pmx_config_t(pkg.MODE_SW, 0, 5, 2, 16, pkg.WANT_SORTED if sorted_ else 0, env["pm"].inner)
    pkg.align_profile_batch_device(cfg, prof, N, pr, dro.data_ptr(), int(np.diff(ro).max()), out.data_ptr(), None,
                                   torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    name = pkg.lib.pmx_last_kernel().decode()
    assert "permtable" in name and "<64,16>" in name, name
    _check(out.cpu().numpy(), _oracle(env, [q] * N, rs), sorted_)


@pytest.mark.parametrize("qlen,shape", [(50, "<8,7>"), (75, "<8,10>"), (100, "<8,13>"), (125, "<8,16>")])
def test_staging_other_read_lengths(env, qlen, shape):
    rng = np.random.default_rng(7107 + qlen)
    qs, rs = random_seqs(rng, N, qlen, qlen), random_seqs(rng, N, qlen - 20, qlen + 20)
    qs[99] = _with(qs[99], 31, ord("N"))
    got, name = _run_pairs(env, qs, rs, qlen & 3)
    assert "permtable" in name and shape in name, name
    _check(got, _oracle(env, qs, rs), qlen)
