"""The bytewise first-hop test of the level-row kernels (lvl_tight_word in
csrc/kernels/spf_device.h, the host build of the function the generic packed
path and the lean kernel call), over every (neighbour byte, own byte) pair in
every byte position of a word, against the scalar rule

    tight  iff  n + 1 == o  and  o != 255

The kernels keep kLvlDirect (254) bytes away from it, so n == o == 254 does
not occur; the rule and the helper agree there anyway (255 != 254) and the
pair is checked with the rest. The increment is bytewise mod 256: n = 255
(unreached from the neighbour) wraps to 0, a level only the source itself
holds - and the kernels force the source's byte to 255 (src_byte), so it
matches nothing. The sweep over all pairs therefore presents an own byte of 0
the way the kernels do, as the source's byte.
"""
import numpy as np
import pytest

from openr_amd import host_module

PAIRS = np.arange(256 * 256, dtype=np.uint32)
N_BYTE, O_BYTE = PAIRS >> 8, PAIRS & 0xFF
NO_SRC = 4  # src_byte outside 0..3: no byte is the source's


def _tight(n, o):
    return ((n + 1 == o) & (o != 255)).astype(np.uint32)


@pytest.fixture(scope="module")
def words():
    return host_module().lvl_tight_words


@pytest.mark.parametrize("pos", range(4))
@pytest.mark.parametrize("fill", [(0, 0), (255, 255), (255, 1), (0, 1), (254, 255), (127, 128), (0x7F, 0xFF)])
def test_every_pair_in_every_byte(words, pos, fill):
    """The pair under test in byte `pos`, the other three bytes a fixed
    (neighbour, own) pair: no carry or borrow leaves a byte either way."""
    fn, fo = (np.uint32(x) * np.uint32(0x01010101) & ~(np.uint32(0xFF) << np.uint32(8 * pos)) for x in fill)
    nw = fn | (N_BYTE << np.uint32(8 * pos))
    ow = fo | (O_BYTE << np.uint32(8 * pos))
    got = np.where(O_BYTE == 0, words(nw, ow, pos), words(nw, ow, NO_SRC))  # level 0: the source's byte
    want = np.zeros_like(PAIRS)
    for k in range(4):
        if k == pos:
            want |= _tight(N_BYTE, O_BYTE) << np.uint32(8 * k)
        else:
            want |= _tight(np.uint32(fill[0]), np.uint32(fill[1])) << np.uint32(8 * k)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(N_BYTE[b]), int(O_BYTE[b]), hex(int(got[b])), hex(int(want[b]))) for b in bad[:8]]


def test_wraps(words):
    """n = 255 against o = 0 is no match once the source's byte is forced
    (own bytes are 0 at the source alone); unforced, the raw wrap matches -
    which is why the kernels force it. n = 254 never pairs with o = 255."""
    for pos in range(4):
        sh = np.uint32(8 * pos)
        nw = np.array([np.uint32(0xFF) << sh], dtype=np.uint32)
        ow = np.array([np.uint32(0)], dtype=np.uint32)
        # the other bytes: n = 0 against o = 0, no match either
        assert int(words(nw, ow, pos)[0]) == 0
        assert int(words(nw, ow, NO_SRC)[0]) == 1 << (8 * pos)
        nw = np.array([np.uint32(0xFE) << sh], dtype=np.uint32)
        ow = np.array([np.uint32(0xFF) << sh], dtype=np.uint32)
        assert int(words(nw, ow, NO_SRC)[0]) == 0


@pytest.mark.parametrize("src", range(4))
def test_forced_source_byte(words, src):
    """Byte `src` of the own word counts as unreached whatever it holds; the
    other bytes are tested as they are."""
    nw = np.full(256, 0x04040404, dtype=np.uint32)  # every neighbour byte 4
    own = np.arange(256, dtype=np.uint32)
    ow = np.uint32(0x05050505) & ~(np.uint32(0xFF) << np.uint32(8 * src)) | (own << np.uint32(8 * src))
    got = words(nw, ow, src)
    want = np.uint32(0x01010101) & ~(np.uint32(0xFF) << np.uint32(8 * src))
    assert np.all(got == want)
