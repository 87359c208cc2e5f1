"""The device PLY reader's rule set, restated in Python integers (test
infrastructure; csrc/slplyread.inl is the code under test).

``parse_body(body, n_rows, n_cols)`` says what sl_parse_ply_ascii must make of
an ASCII body: the status (0 accepted, else which whole-file condition fires),
and for an accepted body ``float(token)`` per token -- Python's float() is
correctly rounded, the exact oracle of the conversion -- with each token's
tier.  Nothing here is floating point except that final float().
"""
from __future__ import annotations

import re

ACCEPTED, BAD_BYTE, BAD_TOKEN, TOKEN_COUNT, RAGGED_LINE, COLOUR_RANGE, UNDECIDED_OVERFLOW = range(7)

WS = b" \t\r\n"
ALPHABET = frozenset(b"0123456789+-.eE" + WS)
TWO53 = 1 << 53
P_MAX = 22
RUN_MAX = 1 << 16  # blanks looked through for a line break before a token

_TOKEN = re.compile(rb"([+-]?)(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?\d+))?\Z")
_SPLIT = re.compile(rb"[^ \t\r\n]+")


def token_parts(tok: bytes):
    """-> (negative, M, p, undecided) by the kernel's accumulation, or None for
    a token outside the grammar.  M stops growing at the digit that would take
    it past 2^53 (undecided: M and p mean nothing then)."""
    m = _TOKEN.match(tok)
    if not m:
        return None
    sign, ip, fp, fp_only, ex = m.groups()
    ip, fp = (ip or b""), (fp_only if fp_only is not None else (fp or b""))
    M, frac, big = 0, 0, False
    for d in ip:
        if M * 10 + (d - 48) > TWO53:
            big = True
            break
        M = M * 10 + (d - 48)
    if not big:
        for d in fp:
            if M * 10 + (d - 48) > TWO53:
                big = True
                break
            M = M * 10 + (d - 48)
            frac += 1
    p = (int(ex) if ex else 0) - frac
    return sign == b"-", M, p, big or abs(p) > P_MAX


def tier(tok: bytes):
    """'exact', 'undecided' or None (outside the grammar)."""
    parts = token_parts(tok)
    return None if parts is None else ("undecided" if parts[3] else "exact")


def exact_tier_value(tok: bytes) -> float:
    """The exact tier's arithmetic: ONE IEEE operation on exact operands."""
    neg, M, p, und = token_parts(tok)
    assert not und
    v = float(M)
    if p < 0:
        v = v / float(10 ** -p)
    elif p > 0:
        v = v * float(10 ** p)
    return -v if neg else v


def reciprocal_shortcut_value(tok: bytes) -> float:
    """What a kernel multiplying by a reciprocal power would give (two roundings)."""
    neg, M, p, und = token_parts(tok)
    assert not und
    v = float(M)
    if p < 0:
        v = v * (1.0 / float(10 ** -p))
    elif p > 0:
        v = v * float(10 ** p)
    return -v if neg else v


def parse_body(body: bytes, n_rows: int, n_cols: int, colour_cols=(), undecided_cap: int = 1 << 16):
    """-> {"status", "values" (float per token, accepted only), "tiers",
    "undecided"}; the conditions in the order the reader tests them."""
    out = {"status": ACCEPTED, "values": None, "tiers": None, "undecided": 0}
    if any(b not in ALPHABET for b in body):
        out["status"] = BAD_BYTE
        return out
    toks = [(m.start(), m.group()) for m in _SPLIT.finditer(body)]
    if len(toks) != n_rows * n_cols:
        out["status"] = TOKEN_COUNT
        return out
    tiers = [tier(t) for _, t in toks]
    if any(t is None for t in tiers):
        out["status"] = BAD_TOKEN
        return out
    for k, (pos, _) in enumerate(toks):  # token k starts a line <=> k % n_cols == 0
        j = pos
        while j > 0 and body[j - 1] in b" \t":
            j -= 1
        starts = j == 0 or body[j - 1] in b"\r\n"
        if pos - j > RUN_MAX or starts != (k % n_cols == 0):
            out["status"] = RAGGED_LINE
            return out
    out["undecided"] = sum(t == "undecided" for t in tiers)
    if out["undecided"] > undecided_cap:
        out["status"] = UNDECIDED_OVERFLOW
        return out
    vals = [float(t) for _, t in toks]
    for c in colour_cols:
        for v in vals[c::n_cols]:
            if not (0 <= v <= 255 and v == int(v)):
                out["status"] = COLOUR_RANGE
                return out
    out["values"], out["tiers"] = vals, tiers
    return out
