"""The masked update of the pair replay's hero-only loop (kernels.hip replay_tapes), on the CPU.

A half that skips a hero-only record does not select `refl` over `refl * m`: the record's product m is replaced, by bit operations
under an all-ones / all-zeros mask, with 1.0, the record is taken as a multiplication, and the loop's unconditional `refl = refl * m`
and `bright = adds ? bright + refl * m : bright` run as for any record. That is the single form's "leave both untouched" iff
x * 1.0 has x's bit pattern for every x the kernel can hold -- f32 with denormals kept, as the kernels are built -- and the bit select
returns exactly one of its two operands. Held here over the special values and random bit patterns. (A signalling NaN comes back quiet;
no f32 operation of the replay makes one.)"""
import numpy as np

ONE = np.float32(1.0).view(np.uint32)


def patterns():
    rng = np.random.default_rng(27)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000, 0xBF800000,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF], dtype=np.uint32)
    return np.concatenate([special, rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])


def is_signalling_nan(bits):
    return ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0) & ((bits & 0x00400000) == 0)


def test_times_one_keeps_every_bit_pattern():
    bits = patterns()
    with np.errstate(all="ignore"):
        product = (bits.view(np.float32) * np.float32(1.0)).view(np.uint32)
    quiet = ~is_signalling_nan(bits)
    assert np.array_equal(product[quiet], bits[quiet])
    assert np.array_equal(product[~quiet], bits[~quiet] | 0x00400000)  # a signalling NaN: the same payload, made quiet


def test_the_bit_select_returns_one_operand():
    """m = (product & ~skip) | (1.0 & skip) and the add / multiply bit (word & ~skip) < 0, skip = 0 - ((word & not_for_me) >> 29)."""
    product = patterns()
    words = np.random.default_rng(28).integers(0, 2 ** 32, product.size, dtype=np.uint64).astype(np.uint32)
    hero_only = np.uint32(1 << 29)
    for not_for_me in (np.uint32(0), hero_only):  # the hero skips nothing; a companion skips the records with bit 29
        skip = (np.uint32(0) - ((words & not_for_me) >> np.uint32(29))).astype(np.uint32)
        skipped = (words & not_for_me) != 0
        assert np.array_equal(skip, np.where(skipped, np.uint32(0xFFFFFFFF), np.uint32(0)))
        m = (product & ~skip) | (ONE & skip)
        assert np.array_equal(m, np.where(skipped, ONE, product))
        adds = (words & ~skip).view(np.int32) < 0
        assert np.array_equal(adds, ~skipped & (words.view(np.int32) < 0))  # a skipped record never adds: it multiplies by 1.0
