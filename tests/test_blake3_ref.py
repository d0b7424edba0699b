"""The from-specification BLAKE3 reference (tests/blake3_ref.py) that the device kernels are
checked against: both of its forms against the published test vectors, against each other
at every chunk count a wave's tree sees, piece decompositions, and the unit assertions of
integrity/blake3.rs:50-132 on the reference itself."""
import pytest

import blake3_ref as R


@pytest.mark.parametrize("n", sorted(R.VECTORS))
def test_known_answers(n):
    data = R.pattern(n)
    assert R.blake3(data).hex() == R.VECTORS[n]
    assert R.blake3_recursive(data).hex() == R.VECTORS[n]


def test_abc():
    assert R.blake3(b"abc").hex() == R.ABC
    assert R.blake3_recursive(b"abc").hex() == R.ABC


def test_recursive_and_levelwise_agree_at_every_chunk_count():
    # 1..130 chunks: every shape of the left-heavy tree up to two waves of chunks, the last
    # chunk partial (even counts) or full (odd counts).  The inputs are prefixes of one
    # pattern, so the plain form's chunk values are shared (memo) and each count costs its
    # own tree.
    memo, memo_cv = {}, {}
    for n in range(1, 131):
        data = R.pattern(n * 1024 - (11 if n % 2 == 0 else 0))
        assert R.blake3(data) == R.blake3_recursive(data, memo), n
        if n % 7 == 1:
            assert R.subtree_cv(data, 3 * 256) == R.subtree_cv_recursive(data, 3 * 256, memo_cv), n


# k = 2 (pieces of 4 chunks): 2..9 pieces, the last of 1, 3 or 4 chunks, the last chunk partial
DECOMPOSITIONS = [(npieces, last, cut) for npieces in range(2, 10) for last, cut in [(1, 0), (3, 0), (4, 1000)]]


@pytest.mark.parametrize("npieces,last,cut", DECOMPOSITIONS)
def test_pieces_joined_equal_one_shot(npieces, last, cut):
    total = (npieces - 1) * 4096 + last * 1024 - cut
    data = R.pattern(total)
    ps = R.pieces(total, 4)
    assert len(ps) == npieces and ps[-1][3] == last
    cvs = [R.subtree_cv(data[o:o + ln], fc) for o, ln, fc, _ in ps]
    assert R.join(cvs) == R.blake3(data) == R.blake3_recursive(data)


def test_first_chunk_enters_the_chaining_value():
    data = R.pattern(4096)
    assert R.subtree_cv(data, 0) != R.subtree_cv(data, 4)
    assert R.subtree_cv(data, 0) != R.blake3(data)  # no ROOT flag


# integrity/blake3.rs:50-132
def test_output_is_32_bytes():
    assert len(R.blake3(b"hello world")) == 32


def test_deterministic():
    assert R.blake3(b"hello world") == R.blake3(b"hello world")


def test_different_inputs_differ():
    assert R.blake3(b"hello world") != R.blake3(b"hello world!")


def test_file_hash_equals_data_hash(tmp_path):
    p = tmp_path / "f"
    payload = b"test content for blake3" * 4000
    p.write_bytes(payload)
    assert R.blake3(p.read_bytes()) == R.blake3(payload)


def test_empty_file_equals_empty_data(tmp_path):
    p = tmp_path / "empty"
    p.write_bytes(b"")
    assert R.blake3(p.read_bytes()) == R.blake3(b"") == bytes.fromhex(R.VECTORS[0])
