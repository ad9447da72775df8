"""The twin of the dictionary encode (tests/dict_encode_ref.py) is tied to the reference and to the decoders before anything is compared
with it: with no dictionary it IS the reference's generic encoder (the oracle's, on inputs of 65 547 bytes and more, where the
reference takes that variant), and every built case's bytes (tests/dict_encode_cases.py) decode to their source through the twin
decoder with the dictionary's tail as history, and through a live liblz4 (LZ4_decompress_safe_usingDict) where there is one."""
import numpy as np
import pytest

import dict_cases
import dict_encode_cases as cases
import dict_encode_ref as ref
import lz4f_ref


def _data(kind, n):
    rng = np.random.default_rng(100 * n + kind)
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == 1:
        return rng.integers(0, 4, n, dtype=np.uint8)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(300)]
    text = b" ".join(words[i] for i in rng.integers(0, 300, n // 3))
    return np.frombuffer(text[:n].ljust(n, b"."), np.uint8)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["random", "four-values", "words"])
@pytest.mark.parametrize("n", [65547, 65847, 70001])
def test_without_a_dictionary_the_twin_is_the_generic_encoder(oracle, n, kind):
    a = _data(kind, n)
    want = bytes(oracle.compress(a))
    assert ref.encode(a.tobytes()) == (len(want), want)
    r = len(want)
    assert ref.encode(a.tobytes(), cap=r) == (r, want) and ref.encode(a.tobytes(), cap=r - 1) == (0, b"")
    assert oracle.compress_raw(a, r)[0] == r and oracle.compress_raw(a, r - 1)[0] == 0


@pytest.mark.parametrize("group", [g for g in cases.GROUPS if g[1] > 0], ids=[i for g, i in zip(cases.GROUPS, cases.IDS) if g[1] > 0])
def test_every_case_decodes_to_its_source(group):
    lz4 = dict_cases.liblz4()
    for c in cases.cases(group):
        r, b = ref.encode(c.block, c.dic.tobytes(), cap=c.cap)
        if r == 0:
            assert ref.encode(c.block, c.dic.tobytes())[0] > c.cap, c.note
            continue
        assert r == len(b) <= c.cap
        assert lz4f_ref.decode_block(b, len(c.block), history=ref.tail_of(c.dic.tobytes())) == (len(c.block), c.block), c.note
        if lz4 is not None:
            assert dict_cases.using_dict(lz4, b, len(c.block), c.dic) == (len(c.block), c.block), c.note


def test_the_primed_table_is_the_highest_position_per_bucket():
    for n in (0, 1, 3, 4, 5, 17, 4097):
        dic = dict_cases.dictionary(n).tobytes()
        table = [0] * ref.TABLE
        for p in range(0, len(dic) - 3):
            table[ref._hash(ref._r32(dic, p))] = p
        assert list(ref.primed_table(dic)) == table
