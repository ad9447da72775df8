"""Pins the CPU oracle (oracle/lz4_oracle.c) against the reference's own C (oracle/_ref/libref_lz4.so): byte-identical
output and identical return codes for the fast encoder (both table variants), LZ4HC, and both decoders, including the
limited-output / wrong-size / corrupted-stream matrix of original/fuzzer.c:176-227.  The reference's answers to the same
calls are recorded in tests/golden/ref_records.json (tests/golden/make_golden.py; the calls are tests/ref_records.py)."""
import ref_records as rr

GOLD = rr.load()


def _check(section, records):
    got, bad = rr.summarise(records)
    assert not bad, (section, "oracle self-check failed (canary overwritten / well-formed stream decoded wrong)", bad[:8])
    want = GOLD[section]
    assert list(got) == list(want), (section, "the cases differ from the recorded ones")
    for g in want:
        assert got[g]["ret"] == want[g]["ret"], (section, g, "return codes", got[g]["ret"], want[g]["ret"])
        assert got[g]["sha"] == want[g]["sha"], (section, g, "bytes differ from the reference's")
    return got


def test_encoders_identical(oracle):
    got = _check("encoders", rr.encoders(oracle, oracle))
    for g, e in got.items():
        assert e["ret"][0] > 0, (g, "compress into compressBound failed")


def test_decoders_identical(oracle):
    _check("decoders", rr.decoders(oracle, oracle))


def test_alignment_independence(oracle):
    # for any block the result must not depend on where the buffer lives: the reference at every offset, and the oracle
    # at every offset, produce the oracle's compress() of the block
    want = oracle.compress(oracle.gen(2, 9, 0, 1, 65536)[0], hc=True)
    got = _check("alignment", rr.alignment(oracle, oracle))
    one = rr.summarise([("", len(want), want, None)])[0][""]
    assert all(e == one for e in got.values()), got


def test_decoders_identical_on_arbitrary_streams(oracle):
    """Streams no encoder produced (tests/stream_fuzz.py: odd but legal sequences, truncated / extended / corrupted /
    zero-offset streams): the restatement and the reference's own C return the same code and the same bytes."""
    _check("streams", rr.streams(oracle))
