"""The PNG row filters and the deflate tokenization of DESIGN.md section 29, restated in numpy / plain Python: what the device
(sniper_amd/csrc/png_encode.hip) must reproduce byte for byte (the filters) or whose output an independent decoder must accept
(the coder).  Nothing here imports the package."""
import numpy as np

FILTER_NAMES = ('None', 'Sub', 'Up', 'Average', 'Paeth')


def paeth_predictor(a, b, c):
    """PNG specification 9.4, elementwise on int arrays: p = a + b - c, the nearest of a, b, c to p, ties in the order a, b, c."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(cur, up, bpp=3):
    """cur, up: the row's bytes and those of the row above (zeros for the first row) -> (5, n) uint8: the row under each filter type."""
    x = np.asarray(cur, np.int64).reshape(-1)
    b = np.asarray(up, np.int64).reshape(-1)
    a = np.concatenate([np.zeros(bpp, np.int64), x[:-bpp]]) if x.size > bpp else np.zeros_like(x)
    c = np.concatenate([np.zeros(bpp, np.int64), b[:-bpp]]) if b.size > bpp else np.zeros_like(b)
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth_predictor(a, b, c)]
    return np.stack([((x - p) & 0xff) for p in preds]).astype(np.uint8)


def filter_cost(v):
    """sum(min(v, 256 - v)) over the filtered bytes"""
    v = np.asarray(v, np.int64)
    return int(np.minimum(v, 256 - v).sum())


def filter_picture(pic, want_types=False):
    """(h, w, 3) uint8 -> the filtered stream, h * (1 + 3w) bytes: per row the type with the smallest cost (ties: the lowest type),
    then the row under it."""
    pic = np.ascontiguousarray(pic, np.uint8)
    h, w, ch = pic.shape
    assert ch == 3
    rows = pic.reshape(h, 3 * w)
    out = np.zeros((h, 1 + 3 * w), np.uint8)
    types = []
    for y in range(h):
        f = filter_row(rows[y], rows[y - 1] if y else np.zeros(3 * w, np.uint8))
        costs = [filter_cost(f[t]) for t in range(5)]
        t = int(np.argmin(costs))           # (argmin: the first of equal minima)
        out[y, 0] = t
        out[y, 1:] = f[t]
        types.append(t)
    return (out.reshape(-1), types) if want_types else out.reshape(-1)


def deflate_bound(n, B):
    """the most bytes the coder writes for a stream of n bytes in blocks of B"""
    nb = -(-n // B)
    return n + 5 * (nb + 1) + 6


def tokens(block):
    """The greedy scan of one block as DESIGN.md section 29 states it: at p >= 1, L = the bytes from p on that equal byte p - 1, capped at 258 and
    the block end; L >= 3 -> ('m', L) and skip L bytes, else ('l', byte).  Distance is always 1."""
    b = bytes(block)
    n, p, out = len(b), 0, []
    while p < n:
        L = 0
        if p >= 1:
            while L < 258 and p + L < n and b[p + L] == b[p - 1]:
                L += 1
        if L >= 3:
            out.append(('m', L))
            p += L
        else:
            out.append(('l', b[p]))
            p += 1
    return out


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def length_symbol(L):
    """RFC 1951 3.2.5: match length -> (symbol, extra bits value, extra bit count)"""
    if L == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if _LEN_BASE[i] <= L)
    return 257 + k, L - _LEN_BASE[k], _LEN_EXTRA[k]


def histogram(toks):
    h = [0] * 286
    for kind, v in toks:
        h[v if kind == 'l' else length_symbol(v)[0]] += 1
    h[256] += 1
    return h


class BitWriter(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def finish(self):
        if self.n:
            self.out.append(self.acc & 0xff)
        self.acc = self.n = 0
        return bytes(self.out)


def pack_dynamic_block(toks, hdr_bits, hdr_words, lens, codes):
    """one dynamic block from the header bits and the (reversed) codes the code construction gave -> bytes, zero bits to the byte end"""
    w = BitWriter()
    for k in range(hdr_bits):
        w.put((hdr_words[k >> 5] >> (k & 31)) & 1, 1)
    for kind, v in toks:
        if kind == 'l':
            w.put(codes[v], lens[v])
        else:
            sym, extra, ne = length_symbol(v)
            w.put(codes[sym], lens[sym])
            w.put(extra, ne)
            w.put(0, 1)
    w.put(codes[256], lens[256])
    return w.finish()


def huffman_depth(counts):
    """the largest depth of a plain (unlimited) Huffman tree over the counts"""
    import heapq
    heap = [(c, i, 0) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return heap[0][2]


def spread(counts):
    """the values 0 .. len(counts) - 1, value v counts[v] times, arranged so that no two equal bytes are adjacent: at every position the
    value with the most occurrences left that differs from the one before (possible while no count exceeds half the total, rounded up)"""
    left = list(counts)
    out, prev = [], -1
    for _ in range(sum(counts)):
        v = max((v for v in range(len(left)) if left[v] and v != prev), key=lambda v: (left[v], -v))
        out.append(v)
        left[v] -= 1
        prev = v
    return np.array(out, np.uint8)
