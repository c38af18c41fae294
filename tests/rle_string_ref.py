"""The two string coders of DESIGN.md section 25 restated in closed form on the host (numpy, no device): what the device kernels are
compared with where the reference itself is not defined (seven-character counts, counts up to 2^32 - 1)."""
import numpy as np

MAX_CHARS = 7


def widths(x):
    """the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1), for every x of an int64 array"""
    x = np.asarray(x, np.int64)
    k = np.ones(x.shape, np.int64)
    for j in range(1, MAX_CHARS):
        lim = np.int64(1) << (5 * j - 1)
        k += ~((x >= -lim) & (x < lim))
    return k


def differences(cnts):
    """x_i = cnts[i] - (i > 2 ? cnts[i-2] : 0) in int64"""
    c = np.asarray(cnts, np.uint32).astype(np.int64)
    x = c.copy()
    x[3:] -= c[1:-2]
    return x


def to_string(cnts):
    """uint32 counts -> str: character j of count i is (((x_i >> 5j) & 0x1f) | (j < k_i - 1 ? 0x20 : 0)) + 48"""
    x = differences(cnts)
    k = widths(x)
    out = bytearray()
    for xi, ki in zip(x.tolist(), k.tolist()):
        for j in range(ki):
            out.append((((xi >> (5 * j)) & 0x1f) | (0x20 if j < ki - 1 else 0)) + 48)
    return out.decode('ascii')


def string_len(cnts):
    return int(widths(differences(cnts)).sum())


def status_of(s):
    """0 ok | 1 the string ends inside a count | 2 a character outside chr(48) .. chr(111) | 3 a count of more than 7 characters; 2
    before 1 before 3 -- and the number of counts (the characters without 0x20)"""
    b = np.frombuffer(s if isinstance(s, bytes) else s.encode('latin-1'), np.uint8).astype(np.int64) - 48
    more = (b & 0x20) != 0
    m = int((~more).sum())
    if ((b < 0) | (b > 63)).any():
        return 2, m
    if len(b) and more[-1]:
        return 1, m
    run = 0
    for v in more.tolist():
        run = run + 1 if v else 0
        if run >= MAX_CHARS:
            return 3, m
    return 0, m


def from_string(s):
    """str -> uint32 counts, modulo 2^32: payloads OR-ed at 5j, sign extension where the last character carries 0x10, then the two
    interleaved prefix sums (odd i; even i >= 2) -- numpy cumsum on uint32 wraps like the kernel's scan"""
    b = np.frombuffer(s if isinstance(s, bytes) else s.encode('ascii'), np.uint8).astype(np.int64) - 48
    last = np.flatnonzero((b & 0x20) == 0)
    assert len(b) == 0 or (len(last) and last[-1] == len(b) - 1), 'the string ends inside a count'
    first = np.concatenate([[0], last[:-1] + 1])
    x = np.zeros(len(last), np.uint64)
    for i, (lo, hi) in enumerate(zip(first.tolist(), last.tolist())):
        k = hi - lo + 1
        v = 0
        for j in range(k):
            v |= int(b[lo + j] & 0x1f) << (5 * j)
        if b[hi] & 0x10:
            v |= -1 << (5 * k)
        x[i] = v & 0xFFFFFFFF
    x = x.astype(np.uint32)
    out = x.copy()
    out[1::2] = np.cumsum(x[1::2], dtype=np.uint32)
    if len(x) > 2:
        out[2::2] = np.cumsum(x[2::2], dtype=np.uint32)
    return out
