"""The adversarial generators (tests/adversarial.py) have the properties the
GPU byte-value tests rely on, and the kernels' byte-SWAR identities hold on
every input -- proven on the CPU.

The second half restates gt_bit7, gt_msb, mask4 and the byte-lane Gray
conversion of csrc/slgpu.hip in NumPy uint32 arithmetic (wrap-around, as the
GPU's) and compares them with the plain comparisons / the oracle's iterated
xor over their whole domain.  A restatement that disagrees with the plain
form means the kernel formula is wrong.
"""
import numpy as np
import pytest

from oracle import sl_oracle as o
from tests import adversarial as adv

U32 = np.uint32


# ----------------------------------------------------------- pair_planes ----

@pytest.fixture(scope="module")
def planes_1k():
    return adv.pair_planes(1024, 1024, 22, seed=1)


def test_pair_planes_cover_every_pair_at_every_residue(planes_1k):
    for k in range(22):
        cov = adv.pair_coverage(planes_1k[2 * k], planes_1k[2 * k + 1])
        assert cov.min() >= 1, f"pair of planes {k}"
    # every pair of planes has its own shuffle
    assert not np.array_equal(planes_1k[0], planes_1k[2])


def test_pair_planes_ragged_frame_covers_every_pair():
    pl = adv.pair_planes(263, 251, 22, seed=5)
    assert pl.shape == (44, 263, 251) and (263 * 251) % 16 == 13
    for k in range(22):
        cov = adv.pair_coverage(pl[2 * k], pl[2 * k + 1]).sum(axis=0)
        assert cov.min() >= 1, f"pair of planes {k}"


def test_pair_planes_are_deterministic():
    a = adv.pair_planes(37, 41, 3, seed=9)
    np.testing.assert_array_equal(a, adv.pair_planes(37, 41, 3, seed=9))
    assert not np.array_equal(a, adv.pair_planes(37, 41, 3, seed=10))
    # a frame below 65536 pixels: a sample of the pairs without repeats
    q = a[0].astype(np.int64).ravel() * 256 + a[1].ravel()
    assert len(np.unique(q)) == q.size


def test_oracle_codes_on_pair_planes_are_uniform_and_out_of_range(planes_1k):
    st = adv.white_black_stack(planes_1k)
    col, row, mask = o.gray_decode_images(list(st), 1920, 1080, o.MASK_ADAPTIVE)
    assert mask.all()
    assert o.gray_decode_images(list(st[:4]), 2, 2, o.MASK_FIXED)[2].all()
    np.testing.assert_array_equal(np.unique(col), np.arange(2048))
    np.testing.assert_array_equal(np.unique(row), np.arange(2048))
    share = (col >= 1920).mean()   # codes the triangulation clips to Wp - 1: 128 / 2048 of a uniform code
    assert 0.055 < share < 0.07, share
    nf, dr = o.adaptive_thresholds(st[0], st[1])
    assert (nf, dr) == (0.0, 255.0) and adv.int_thresholds(nf, dr) == (0, 12)


# ------------------------------------------------------------ mask_frame ----

# the oracle mask's share of the frame on the dense rows of adv.MASK_CASES
MASK_SHARE = {(0, 255): 0.93, (37, 100): 0.77, (85, 255): 0.49, (86, 255): 0.49, (10, 21): 0.92, (10, 20): 0.92,
              (10, 19): 0.92}


@pytest.mark.parametrize("v_pad,D,tw,tc,empty", adv.MASK_CASES)
def test_mask_frame_thresholds_and_edges(v_pad, D, tw, tc, empty):
    white, black = adv.mask_frame(2560, 2560, v_pad, D, seed=3)
    nf, dr = o.adaptive_thresholds(white, black)
    assert nf == v_pad and dr == D
    assert adv.int_thresholds(nf, dr) == (tw, tc)
    mask = o.valid_mask(white, black)
    wi, bi = white.astype(np.int32), black.astype(np.int32)
    np.testing.assert_array_equal(mask, (wi > tw) & (wi - bi > tc))
    edges = adv.edge_counts(white, black, tw, tc)
    print(f"v_pad {v_pad} D {D}: mask {mask.mean():.4f}, min edge count {edges.min()}")
    if empty:
        assert not mask.any()
    else:
        assert mask.any() and not mask.all()
        assert edges.min() >= 1, edges
    if (v_pad, D) in MASK_SHARE:
        assert abs(mask.mean() - MASK_SHARE[(v_pad, D)]) < 0.01


def test_mask_frame_ragged():
    white, black = adv.mask_frame(2563, 2561, 37, 100, seed=4)
    assert (2563 * 2561) % 16 != 0
    assert o.adaptive_thresholds(white, black) == (37.0, 100.0)
    assert adv.edge_counts(white, black, 55, 5).min() >= 1


# ---------------------------------------------------------- sparse_masks ----

def test_sparse_masks():
    H, W = 65, 128
    m = adv.sparse_masks(H, W)
    n = H * W
    assert n % adv.CHUNK != 0 and W % 16 == 0
    flat = {k: v.ravel() for k, v in m.items()}
    chunks = -(-n // adv.CHUNK)
    assert flat["all_true"].all() and not flat["all_false"].any()
    assert np.flatnonzero(flat["first_pixel"]).tolist() == [0]
    assert np.flatnonzero(flat["last_pixel"]).tolist() == [n - 1]
    assert np.flatnonzero(flat["first_of_every_chunk"]).tolist() == [adv.CHUNK * c for c in range(chunks)]
    assert np.flatnonzero(flat["last_of_every_chunk"]).tolist() == \
        [min(adv.CHUNK * (c + 1), n) - 1 for c in range(chunks)]
    np.testing.assert_array_equal(flat["full_but_last_of_every_chunk"], ~flat["last_of_every_chunk"])
    full = flat["full_but_last_of_every_chunk"][: adv.CHUNK]
    assert full.sum() == adv.CHUNK - 1
    for k in (2, 3, 4, 64):
        assert np.flatnonzero(flat[f"period_{k}"]).tolist() == list(range(0, n, k))
    per_chunk = [int(flat["alternating_chunks"][adv.CHUNK * c: adv.CHUNK * (c + 1)].sum()) for c in range(chunks)]
    assert per_chunk == [adv.CHUNK if c % 2 == 0 else 0 for c in range(chunks - 1)] + [n % adv.CHUNK]
    assert len(m) == 12
    for name, mk in m.items():   # mask_stack realises the mask under the fixed thresholds
        st = adv.mask_stack(mk, np.zeros((2, H, W), np.uint8))
        np.testing.assert_array_equal(o.valid_mask(st[0], st[1], o.MASK_FIXED), mk, err_msg=name)


# ---------------------------------- NumPy restatements of the SWAR routines ----

H80 = U32(0x80808080)


def bitop3(a, b, c, table):
    """v_bitop3_b32: per bit, bit (4 a + 2 b + c) of the 8-bit truth table."""
    out = np.zeros_like(a)
    for idx in range(8):
        if (table >> idx) & 1:
            term = (a if idx & 4 else ~a) & (b if idx & 2 else ~b) & (c if idx & 1 else ~c)
            out |= term
    return out


def gt_bit7(a, b):
    d = (b | H80) - (a & ~H80)
    return bitop3(a, b, d, 0x71), d


def gt_msb(a, b):
    low = (a | H80) - ((b & ~H80) + U32(0x01010101))
    return ((a & ~b) | (~(a ^ b) & low)) & H80


def mask4(w, b, tw, tc):
    """-> (bit e = pixel e valid, the 0 / 1 mask bytes) as csrc/slgpu.hip's
    mask4 and k_count's vector branch compute them."""
    tw2 = U32((tw + 1) & 0xFFFFFFFF) * U32(0x00010001)
    tc2 = U32((tc + 17) & 0xFFFFFFFF) * U32(0x00010001)
    L, T, S = U32(0x00FF00FF), U32(0x80008000), U32(0x00100010)
    we, wo = w & L, (w >> U32(8)) & L
    be, bo = b & L, (b >> U32(8)) & L
    me = ((we | T) - tw2) & (((we + S) | T) - (be + tc2))
    mo = ((wo | T) - tw2) & (((wo + S) | T) - (bo + tc2))
    y = ((me >> U32(15)) & U32(0x00010001)) | ((mo >> U32(7)) & U32(0x01000100))
    bits = (y & U32(1)) | ((y >> U32(7)) & U32(2)) | ((y >> U32(14)) & U32(4)) | ((y >> U32(21)) & U32(8))
    return bits, y


def bitreverse32(x):
    x = ((x >> U32(1)) & U32(0x55555555)) | ((x & U32(0x55555555)) << U32(1))
    x = ((x >> U32(2)) & U32(0x33333333)) | ((x & U32(0x33333333)) << U32(2))
    x = ((x >> U32(4)) & U32(0x0F0F0F0F)) | ((x & U32(0x0F0F0F0F)) << U32(4))
    x = ((x >> U32(8)) & U32(0x00FF00FF)) | ((x & U32(0x00FF00FF)) << U32(8))
    return (x >> U32(16)) | (x << U32(16))


def gray_to_binary_bytes(x, bits):
    if bits > 1:
        x = x ^ ((x >> U32(1)) & U32(0x7F7F7F7F))
    if bits > 2:
        x = x ^ ((x >> U32(2)) & U32(0x3F3F3F3F))
    if bits > 4:
        x = x ^ ((x >> U32(4)) & U32(0x0F0F0F0F))
    return x


def decode_words(P, I, n):
    """k_decode's code of 4 packed pixels per word from k = len(P) (pattern,
    inverse) word pairs of an n-bit code: gt_bit7, the shifting byte-lane
    accumulators A (pairs 0..7) and B, bitreverse, the byte-lane Gray
    conversion with A's parity carried into B, and the shift of a truncated
    stack.  -> int64 [words, 4] (pixel 4 w + e at [w, e])."""
    k = len(P)
    A = np.zeros_like(P[0])
    B = np.zeros_like(P[0])
    for pair in range(k):
        g = gt_bit7(P[pair], I[pair])[0]
        if pair < 8:
            A = ((A >> U32(1)) & U32(0x7F7F7F7F)) | (g & H80)
        else:
            B = ((B >> U32(1)) & U32(0x7F7F7F7F)) | (g & H80)
    kA = min(k, 8)
    kB = k - kA
    A = gray_to_binary_bytes(bitreverse32(A), kA)
    B = gray_to_binary_bytes(bitreverse32(B) ^ ((A & U32(0x01010101)) << U32(kB - 1)), kB) if kB > 0 \
        else np.zeros_like(A)
    out = np.empty((len(A), 4), np.int64)
    for e in range(4):
        sft = U32(8 * (3 - e))
        c = (((A >> sft) & U32(0xFF)) << U32(kB)) | ((B >> sft) & U32(0xFF))
        sh = n - k
        if sh > 0:
            lo = c & U32(1)
            c = (c << U32(sh)) | ((lo << U32(sh)) - lo)
        out[:, e] = c
    return out


def _words_with_all_pairs(rng):
    """uint32 a, b [65536] and the byte values [65536, 4]: byte lane k of the
    words runs over all 65536 (x, y) byte pairs in its own shuffled order, so
    every pair meets random neighbour bytes."""
    xs = np.empty((N := 65536, 4), np.uint32)
    ys = np.empty((N, 4), np.uint32)
    for k in range(4):
        q = rng.permutation(N).astype(np.uint32)
        xs[:, k], ys[:, k] = q >> 8, q & 255
    sh = (U32(8) * np.arange(4, dtype=np.uint32))[None, :]
    return (xs << sh).sum(axis=1, dtype=np.uint32), (ys << sh).sum(axis=1, dtype=np.uint32), xs, ys


def test_truth_table_0x71_is_the_comment_boolean():
    rng = np.random.default_rng(0)
    a, b, d = (rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    np.testing.assert_array_equal(bitop3(a, b, d, 0x71), ~((b & ~a) | (~(a ^ b) & d)))
    # the documented derivation of the table: src0 = 0xf0, src1 = 0xcc, src2 = 0xaa
    s0, s1, s2 = 0xF0, 0xCC, 0xAA
    assert (~((s1 & ~s0) | (~(s0 ^ s1) & s2))) & 0xFF == 0x71


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_byte_compares_on_every_pair_with_random_neighbours(seed):
    rng = np.random.default_rng(seed)
    a, b, xs, ys = _words_with_all_pairs(rng)
    want = xs > ys
    with np.errstate(over="ignore"):
        g7, d = gt_bit7(a, b)
        gm = gt_msb(a, b)
    for k in range(4):
        np.testing.assert_array_equal(((g7 >> U32(8 * k + 7)) & U32(1)).astype(bool), want[:, k])
        np.testing.assert_array_equal(((gm >> U32(8 * k + 7)) & U32(1)).astype(bool), want[:, k])
        # the comment's range claim: no borrow leaves a byte
        dk = (d >> U32(8 * k)) & U32(0xFF)
        np.testing.assert_array_equal(dk, (ys[:, k] | 0x80) - (xs[:, k] & 0x7F))
        assert dk.min() >= 1
    assert not (gm & ~H80).any()


def _mask4_check(w, b, ws, bs, tw, tc):
    with np.errstate(over="ignore"):
        bits, y = mask4(w, b, tw, tc)
    want = (ws > tw) & (ws - bs > tc)
    for e in range(4):
        assert np.array_equal(((bits >> U32(e)) & U32(1)).astype(bool), want[:, e]), (tw, tc, e)
        assert np.array_equal((y >> U32(8 * e)) & U32(0xFF), want[:, e].astype(np.uint32)), (tw, tc, e)


def test_mask4_on_every_pair_and_threshold():
    """All (w, b) byte pairs at every byte position, for every tc in [-17, 12]
    at tw in {-1, 0, 127, 128, 255, 382} and every tw in [-1, 382] at tc in
    {-13, 0, 12}: the documented exact range of the 16-bit-lane compares (k_count
    takes the SWAR branch for tw >= -1, tc >= -17) and beyond what the adaptive
    recipe reaches (tw in [0, 382], tc in [-13, 12])."""
    rng = np.random.default_rng(7)
    w, b, ws, bs = _words_with_all_pairs(rng)
    ws, bs = ws.astype(np.int64), bs.astype(np.int64)
    for tw in (-1, 0, 127, 128, 255, 382):
        for tc in range(-17, 13):
            _mask4_check(w, b, ws, bs, tw, tc)
    for tc in (-13, 0, 12):
        for tw in range(-1, 383):
            _mask4_check(w, b, ws, bs, tw, tc)
    _mask4_check(w, b, ws, bs, 40, 10)   # the fixed thresholds


@pytest.mark.parametrize("n", range(1, 17))
def test_byte_lane_gray_conversion_every_width(n):
    """n-bit codes from k <= n (pattern, inverse) pairs, every Gray value of
    the k bits, against the oracle's decode_sequence (iterated xor to a fixed
    point, sl_system.py:544-572) on the same planes: the A-only, A + B and
    shifted cases of k_decode."""
    rng = np.random.default_rng(n)
    for k in range(1, n + 1):
        npx = max(1 << k, 4)
        g = np.arange(npx, dtype=np.int64) & ((1 << k) - 1)
        # pair j carries Gray bit k - 1 - j: pattern > inverse where it is set
        imgs = []
        for j in range(k):
            bit = ((g >> (k - 1 - j)) & 1).astype(bool)
            lo = rng.integers(0, 255, npx)
            hi = lo + 1 + (rng.integers(0, 256, npx) % (255 - lo))
            inv = np.where(rng.random(npx) < 0.3, lo, hi)   # ties decode as 0 (strict >)
            imgs += [np.where(bit, hi, lo).astype(np.uint8)[None], np.where(bit, lo, inv).astype(np.uint8)[None]]
        want, idx = o._decode_sequence(imgs, 0, n)
        assert idx == 2 * k
        words = [im.ravel().view(np.uint32) for im in imgs]   # little endian: pixel e in byte e
        with np.errstate(over="ignore"):
            got = decode_words(words[0::2], words[1::2], n)
        np.testing.assert_array_equal(got.ravel(), want.ravel(), err_msg=f"{k} pairs of {n} bits")
