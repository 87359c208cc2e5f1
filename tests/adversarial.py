"""Adversarial input generators for the decode and mask kernels (NumPy, seeded).

A rendered stack has a narrow byte distribution (lit ~ albedo * 200 + ambient,
unlit <= ~20), so it never reaches most of the byte-value pairs the kernels'
byte-SWAR compares are defined on.  These generators do:

* ``pair_planes``  -- (pattern, inverse) planes that carry every ordered byte
  pair (p, i) at every byte position of a lane's 16-byte load;
* ``mask_frame``   -- a white / black frame with exact, chosen adaptive
  thresholds and every (white, black) pair around them at every byte position
  of a word;
* ``sparse_masks`` -- the validity masks at the edges of the 1024-pixel chunk
  compaction.

tests/test_adversarial_inputs.py proves these properties on the CPU;
tests/test_gpu_byte_values.py feeds the arrays to the kernels.
"""
import numpy as np

CHUNK = 1024      # pixels per compaction chunk (csrc/slgpu.hip: kChunk)
N_PAIRS = 65536   # ordered byte pairs
MASK_BLOCK_SHARE = 0.05  # mask_frame: the exhaustive block's largest share of the frame

# (v_pad, D) -> (tw, tc): the adaptive integer thresholds white > tw,
# white - black > tc of a mask_frame(H, W, v_pad, D, seed) frame.  nf = v_pad and
# dr = D exactly; tw = floor(f32(nf) * 1.5), tc = floor(f32(dr) * f32(0.05))
# (sl_system.py:526-535; white and contrast are integers).
MASK_CASES = [
    # v_pad, D, tw, tc, empty
    (0, 255, 0, 12, False),
    (37, 100, 55, 5, False),
    (85, 255, 127, 12, False),
    (86, 255, 129, 12, False),
    (169, 60, 253, 3, False),
    (10, 21, 15, 1, False),
    (10, 20, 15, 1, False),     # float32 20 * 0.05 rounds to 1.0
    (10, 19, 15, 0, False),
    (10, 1, 15, 0, False),
    (10, 0, 15, 0, True),
    (255, 255, 382, 12, True),
    (40, -7, 60, -1, True),
]


def _all_pairs_shuffled(rng, m):
    """m values of a seeded shuffle of the 65536 pair indices, tiled when
    m > 65536 (every index then occurs floor(m / 65536) times or once more)."""
    base = np.arange(max(m, N_PAIRS), dtype=np.uint32) & 0xFFFF
    return rng.permutation(base)[:m].astype(np.uint16)


def pair_planes(H, W, n_pairs, seed):
    """uint8 [2 * n_pairs, H, W]: planes 2k, 2k + 1 are a (pattern, inverse)
    pair.  With H * W >= 16 * 65536 the pixels of each residue j = index % 16
    (the byte position in a lane's 16-byte load) carry a shuffle of all 65536
    ordered byte pairs (p, i), tiled; with 65536 <= H * W < 16 * 65536 the
    frame as a whole carries such a shuffle (the residues sample it); below
    that the pairs are a sample without repeats.  Every pair of planes gets
    its own shuffle, so the decoded bits are independent and the codes
    uniform."""
    n = H * W
    rng = np.random.default_rng(seed)
    out = np.empty((2 * n_pairs, n), np.uint8)
    for k in range(n_pairs):
        q = np.empty(n, np.uint16)
        if n // 16 >= N_PAIRS:
            for j in range(16):
                q[j::16] = _all_pairs_shuffled(rng, len(range(j, n, 16)))
        else:
            q[:] = _all_pairs_shuffled(rng, n)
        out[2 * k] = q >> 8
        out[2 * k + 1] = q & 255
    return out.reshape(2 * n_pairs, H, W)


def pair_coverage(P, I):
    """Occurrences of every (residue, p, i) triple: int array [16, 256, 256]."""
    n = P.size
    key = (np.arange(n, dtype=np.int64) % 16) * N_PAIRS + P.ravel().astype(np.int64) * 256 + I.ravel()
    return np.bincount(key, minlength=16 * N_PAIRS).reshape(16, 256, 256)


def mask_frame(H, W, v_pad, D, seed):
    """(white, black) uint8 [H, W] whose adaptive thresholds are exactly
    np.percentile(black, 95) == v_pad and max(white - black) == D.

    An exhaustive block holds every pair (w, b) with w - b <= D once at each of
    the 4 byte positions of a word (its own shuffle per position), at seeded
    word-aligned positions of the flattened frame; where that would exceed
    MASK_BLOCK_SHARE of the frame, a seeded sample of the pairs that keeps
    those with w - b == D.  Every other pixel has black = v_pad and white =
    min(random byte, clip(v_pad + D, 0, 255)): at least 95 % of the black
    plane is v_pad, with fewer than 5 % above it, so both neighbours of the
    percentile's virtual index are v_pad."""
    n = H * W
    rng = np.random.default_rng(seed)
    w = np.repeat(np.arange(256), 256)
    b = np.tile(np.arange(256), 256)
    keep = (w - b) <= D
    w, b = w[keep], b[keep]
    if len(w) == 0:
        raise ValueError(f"no byte pair has white - black <= {D}")
    m = len(w)
    if 4 * m > MASK_BLOCK_SHARE * n:
        raise ValueError(f"a {H}x{W} frame is too small: the block would exceed {MASK_BLOCK_SHARE:.0%} of it")
    white = np.minimum(rng.integers(0, 256, n), int(np.clip(v_pad + D, 0, 255))).astype(np.uint8)
    black = np.full(n, v_pad, np.uint8)
    pos = rng.permutation(n // 4)[:m] * 4
    for j in range(4):
        sel = rng.permutation(m)
        white[pos + j] = w[sel]
        black[pos + j] = b[sel]
    return white.reshape(H, W), black.reshape(H, W)


def int_thresholds(nf, dr):
    """The integer thresholds of float32 (noise_floor, dynamic_range):
    x > f32(nf) * 1.5 <=> x > tw and x > f32(dr) * 0.05 <=> x > tc for
    integer x."""
    tw = int(np.floor(np.float32(nf) * np.float32(1.5)))
    tc = int(np.floor(np.float32(dr) * np.float32(0.05)))
    return tw, tc


def edge_counts(white, black, tw, tc):
    """int [4, 4]: per byte position of a word (flat index % 4), the pixels
    with w == tw, w == tw + 1, w - b == tc, w - b == tc + 1."""
    wi = white.ravel().astype(np.int32)
    ci = wi - black.ravel().astype(np.int32)
    pos = np.arange(wi.size) % 4
    out = np.empty((4, 4), np.int64)
    for j in range(4):
        s = pos == j
        out[j] = [(wi[s] == tw).sum(), (wi[s] == tw + 1).sum(), (ci[s] == tc).sum(), (ci[s] == tc + 1).sum()]
    return out


def sparse_masks(H, W):
    """name -> bool [H, W]: the validity masks at the compaction's edges (a
    chunk is CHUNK consecutive pixels of the flattened frame; the frame's last
    chunk may be partial, its last pixel is then the frame's last)."""
    n = H * W
    i = np.arange(n)
    last_of_chunk = (i % CHUNK == CHUNK - 1) | (i == n - 1)
    m = {
        "all_true": np.ones(n, bool),
        "all_false": np.zeros(n, bool),
        "first_pixel": i == 0,
        "last_pixel": i == n - 1,
        "first_of_every_chunk": i % CHUNK == 0,
        "last_of_every_chunk": last_of_chunk,
        "full_but_last_of_every_chunk": ~last_of_chunk,
        "period_2": i % 2 == 0,
        "period_3": i % 3 == 0,
        "period_4": i % 4 == 0,
        "period_64": i % 64 == 0,
        "alternating_chunks": (i // CHUNK) % 2 == 0,
    }
    return {k: v.reshape(H, W) for k, v in m.items()}


def mask_stack(mask, planes):
    """A stack whose fixed-threshold mask (white > 40, white - black > 10) is
    ``mask``: white 255 / black 0 where true, white 0 / black 0 where false,
    then the bit planes."""
    white = np.where(mask, 255, 0).astype(np.uint8)
    return np.concatenate([white[None], np.zeros_like(white)[None], planes])


def white_black_stack(planes):
    """white = 255, black = 0, then the bit planes: every pixel valid under
    both mask modes (adaptive: nf 0, dr 255 -> white > 0, contrast > 12)."""
    H, W = planes.shape[-2:]
    return np.concatenate([np.full((1, H, W), 255, np.uint8), np.zeros((1, H, W), np.uint8), planes])
