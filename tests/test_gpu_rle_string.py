"""-m gpu: sn_rle_string_len / sn_rle_to_string / sn_rle_string_count / sn_rle_from_string against the reference's own strings
(tests/golden/cocoresults_v1.npz) and, where the reference is not defined (seven-character counts, counts up to 2^32 - 1), against the
closed-form restatement (tests/rle_string_ref.py).  Every operand sits between guard bytes, two runs give the same bytes, and there
is no tolerance anywhere: everything is bytes."""
import numpy as np
import pytest

import coco_results_util as RU
import rle_string_ref as ref

pytestmark = pytest.mark.gpu

BOUNDARIES = (15, 511, 16383, 2 ** 19 - 1, 2 ** 24 - 1, 2 ** 29 - 1)          # x and x + 1 take k and k + 1 characters; -x - 1 and -x - 2


@pytest.fixture(scope='module')
def golden():
    return RU.load_golden()


@pytest.fixture(scope='module')
def limits():
    from sniper_amd.results import rle_string_limits
    return rle_string_limits()


def _from_differences(x, start):
    """a count array whose coded differences from the fourth count on are x (chains of both parities started at `start`)"""
    c = [1, start, start]
    for v in x:
        c.append(c[-2] + int(v))
    assert min(c) >= 0 and max(c) < 2 ** 32
    return np.array(c, np.uint32)


def _seeded(rng, m, wide=False):
    """m counts with differences of every width; wide: up to 2^32 - 1"""
    mag = rng.randint(0, 7 if wide else 6, m)
    c = rng.randint(0, 2 ** 32, m, dtype=np.uint64) % (np.uint64(32) ** (mag + 1).astype(np.uint64) * np.uint64(4 if wide else 8))
    return np.minimum(c, 2 ** 32 - 1).astype(np.uint32)


def _check_both_ways(rles):
    want = [ref.to_string(c).encode('ascii') for c in rles]
    got, lens = RU.device_encode(rles)
    assert lens.tolist() == [len(w) for w in want]
    assert got == want
    back, m, status = RU.device_decode(got)
    assert m.tolist() == [len(c) for c in rles] and not status.any()
    for b, c in zip(back, rles):
        assert np.array_equal(b, c)
    return got


def test_limits(limits):
    assert limits == {'threads': 64, 'chunk': 64, 'max_chars': 7}


def test_golden_both_directions(golden):
    from sniper_amd.evaluation import rle_from_string
    got, lens = RU.device_encode(golden['counts'])
    assert [g.decode('ascii') for g in got] == golden['strings']
    back, m, status = RU.device_decode(golden['strings'])
    assert not status.any() and m.tolist() == [len(c) for c in golden['counts']]
    for b, c, s in zip(back, golden['counts'], golden['strings']):
        assert np.array_equal(b, c) and np.array_equal(b, rle_from_string(s))
    assert RU.device_encode(golden['counts'])[0] == got                         # a second run: the same bytes


@pytest.mark.parametrize('batch', (1, 2, 65))
def test_every_seam_in_batches(limits, batch):
    """m = 1 .. 4 (no chain, the first links of both chains), the wave and chunk seams, two chunks and one: the carry of the
    positions and of both parity chains"""
    T = limits['chunk']
    sizes = sorted({1, 2, 3, 4, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1})
    rng = np.random.RandomState(100 + batch)
    for m in sizes:
        rles = [_seeded(rng, m) for _ in range(batch)]
        if batch > 2:
            rles[batch // 2] = np.zeros(0, np.uint32)                           # a mask without counts among the others
            rles[-1] = _seeded(rng, 3 * T + 2)
        _check_both_ways(rles)


def test_every_width_and_boundary_with_both_signs():
    xs = []
    for b in BOUNDARIES:
        xs += [b, b + 1, -b - 1, -b - 2]
    chain = xs + [0, -1, 2 ** 31 - 1, 2 ** 31 - 8]
    xs += [0, -1, 2 ** 31 - 1, -2 ** 31]
    rles = [_from_differences([x], 2 ** 31) for x in xs]
    rles.append(_from_differences(chain, 2 ** 31))                              # and in two chains that end just below 2^32
    strings = _check_both_ways(rles)
    for x, s in zip(xs, strings):
        k = int(ref.widths(np.array([x]))[0])
        assert len(s) == 1 + 7 + 7 + k, (x, s)                                  # 1, 2^31, 2^31 then x
    assert sorted({int(ref.widths(np.array([x]))[0]) for x in xs}) == [1, 2, 3, 4, 5, 6, 7]
    assert {(int(ref.widths(np.array([x]))[0]), x < 0) for x in xs} >= {(k, neg) for k in range(1, 8) for neg in (False, True)}


def test_counts_up_to_the_last_uint32():
    rng = np.random.RandomState(7)
    top = 2 ** 32 - 1
    rles = [np.array([top], np.uint32), np.array([0, top], np.uint32), np.array([top, 0, top, 0, top, 0, top], np.uint32),
            np.array([0, top, 0, 0, top, top, 1, 0], np.uint32)] + [_seeded(rng, m, wide=True) for m in (5, 64, 65, 200)]
    strings = _check_both_ways(rles)
    assert any(len(s) > 6 * len(c) for s, c in zip(strings, rles))              # past what the reference allocates


def test_bad_strings_among_good_ones(golden):
    from sniper_amd.evaluation import rle_from_string
    from sniper_amd.results import rle_from_strings
    good = golden['strings'][:6] + ['', '0']
    long8 = ref.to_string(np.array([3, 7], np.uint32)) + 'PPPPPPP1' + 'Q0'      # a count of eight characters: 1 << 35 is gone modulo 2^32
    long9 = 'oooooooo0' + ref.to_string(np.array([9, 9, 9, 9], np.uint32))      # nine, with payload bits that count
    bad = {2: ('0P', 1), 4: ('0:~1', 2), 5: (long8, 3), 7: ('PPPPPPPP', 1), 9: ('/0', 2), 10: (long9, 3), 11: ('~' + 'P' * 9, 2)}
    strings = list(good)
    for at in sorted(bad):
        strings.insert(at, bad[at][0])
    back, m, status = RU.device_decode(strings)
    for n, s in enumerate(strings):
        assert (int(status[n]), int(m[n])) == ref.status_of(s), (n, s)
        if n in bad:
            assert status[n] == bad[n][1] and (back[n] == 0xA5A5A5A5).all(), (n, s)          # flagged, and nothing written
        else:
            assert status[n] == 0 and np.array_equal(back[n], rle_from_string(s)), (n, s)
    # the Python surface: status 3 falls back to the host and equals rle_from_string; 1 and 2 raise, naming the first
    ok = [s for n, s in enumerate(strings) if n not in bad or bad[n][1] == 3]
    out = rle_from_strings(ok)
    assert len(out) == len(ok)
    for s, o in zip(ok, out):
        assert o.dtype == np.uint32 and np.array_equal(o, rle_from_string(s)), s
    assert sum(ref.status_of(s)[0] == 3 for s in ok) == 2
    with pytest.raises(ValueError) as e:
        rle_from_strings(strings)
    assert 'string 2' in str(e.value) and 'rle_from_string: the string ends inside a count' in str(e.value)
    with pytest.raises(ValueError) as e:
        rle_from_strings(strings[3:])
    assert 'string 1' in str(e.value) and 'outside chr(48) .. chr(111)' in str(e.value)


def test_slots_that_do_not_fit_are_never_overrun():
    """offsets that pass the entry points' checks but are not the ones the length pass gives: a mask writes what fits into its own
    slots [off[n], off[n+1]) and nothing else -- the neighbours' bytes, the spare bytes and the guards stay as they were"""
    import torch
    from coco_eval_util import Guarded
    from sniper_amd import hip
    rng = np.random.RandomState(11)
    rles = [_seeded(rng, m, wide=True) for m in (70, 130, 5)]
    want = [ref.to_string(c).encode('ascii') for c in rles]
    run_off = RU.offsets([len(c) for c in rles])
    slots = [len(want[0]) + 2, len(want[1]) - 3, len(want[2])]                 # two spare bytes, three too few, exact
    str_off = RU.offsets(slots)
    G = Guarded()
    d_c, d_roff, d_soff = G.put(np.concatenate(rles)), G.put(run_off), G.put(str_off)
    o_s = G.put(np.full(int(str_off[-1]), 0xEE, np.uint8))
    G.items[-1] = (G.items[-1][0], G.items[-1][1], None)
    hip.call('sn_rle_to_string', d_c, d_roff, run_off, d_soff, str_off, 3, int(run_off[-1]), int(str_off[-1]), o_s, hip.stream())
    torch.cuda.synchronize()
    G.check()
    got = Guarded.read(o_s, (int(str_off[-1]),), np.uint8).tobytes()
    assert got == want[0] + b'\xee\xee' + want[1][:-3] + want[2]
    # the decoder: the counts of string 1 get two slots too few
    m = [len(c) for c in rles]
    short_off = RU.offsets([m[0], m[1] - 2, m[2]])
    true_soff = RU.offsets([len(w) for w in want])
    G = Guarded()
    d_s, d_soff, d_roff = G.put(np.frombuffer(b''.join(want), np.uint8)), G.put(true_soff), G.put(short_off)
    d_st = G.put(np.zeros(3, np.int32))
    o_c = G.out((int(short_off[-1]),), np.uint32)
    hip.call('sn_rle_from_string', d_s, d_soff, true_soff, d_roff, short_off, d_st, 3, int(true_soff[-1]), int(short_off[-1]), o_c, hip.stream())
    torch.cuda.synchronize()
    G.check()
    back = Guarded.read(o_c, (int(short_off[-1]),), np.uint32)
    assert np.array_equal(back, np.concatenate([rles[0], rles[1][:-2], rles[2]]))


def test_python_surface_and_two_runs(golden):
    from sniper_amd.results import rle_from_strings, rle_to_strings
    rng = np.random.RandomState(3)
    rles = list(golden['counts']) + [_seeded(rng, m, wide=True) for m in (1, 70, 130)] + [np.zeros(0, np.uint32)]
    a = rle_to_strings(rles)
    assert a[:len(golden['strings'])] == golden['strings'] and a == [ref.to_string(c) for c in rles]
    assert rle_to_strings([{'size': [1, 1], 'counts': c} for c in rles]) == a
    back = rle_from_strings(a)
    assert all(b.dtype == np.uint32 and np.array_equal(b, c) for b, c in zip(back, rles))
    again = rle_from_strings([s.encode('ascii') for s in a])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(back, again))
    assert rle_to_strings([]) == [] and rle_from_strings([]) == []
