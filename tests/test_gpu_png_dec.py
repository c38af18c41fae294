"""GPU: zlib streams inflated on the device, PNG files decoded on top of that, and the VOC ground truth cut from index maps
(sniper_amd/png_decode.py, sniper_amd/voc_gt.py; csrc/png_decode.hip, csrc/inflate_code.h, csrc/voc_gt.hip).  Every output has an exact
host oracle: zlib.decompress, PIL, and the numpy restatements of tests/png_dec_ref.py; all comparisons are == / np.array_equal."""
import io
import os
import zlib

import numpy as np
import pytest

import png_dec_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dec():
    from sniper_amd import png_decode as mod
    return mod


@pytest.fixture(scope='module')
def streams():
    return ref.stream_set()


def _inflate_exact(dec, items, slack=0):
    outs, lengths, status = dec.inflate_streams([s for _, s, _ in items], [len(d) + slack for _, _, d in items])
    assert len(outs) == len(items) and status.tolist() == [0] * len(items), dict(zip([n for n, _, _ in items], status.tolist()))
    for (name, _, data), o, n in zip(items, outs, lengths):
        assert int(n) == len(data) and o.cpu().numpy().tobytes() == data, name


# ---- inflate ---------------------------------------------------------------------------------------------------------------------
def test_inflate_equals_zlib_on_the_stream_set_in_one_batch(dec, streams):
    for _, s, d in streams:
        assert zlib.decompress(s) == d
    _inflate_exact(dec, streams)
    _inflate_exact(dec, streams[::-1], slack=3)          # another order, capacities above the lengths


def test_inflate_batches_of_1_and_of_65(dec, streams):
    for item in (streams[0], streams[4], [s for s in streams if s[0] == 'far'][0]):
        _inflate_exact(dec, [item])
    small = [s for s in streams if len(s[2]) <= 9000]
    batch = [small[i % len(small)] for i in range(65)]
    _inflate_exact(dec, batch)


def test_inflate_takes_one_device_buffer_with_offsets(dec, streams):
    import torch
    items = streams[:6]
    flat = np.frombuffer(b''.join(s for _, s, _ in items), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in items])]).astype(np.int64)
    outs, lengths, status = dec.inflate_streams(torch.from_numpy(flat.copy()).cuda(), [len(d) for _, _, d in items], offsets=off)
    assert status.tolist() == [0] * 6 and [o.cpu().numpy().tobytes() for o in outs] == [d for _, _, d in items]
    with pytest.raises(ValueError):
        dec.inflate_streams([b'x'], [1, 2])


def test_damaged_streams_give_their_status_and_leave_their_neighbours_exact(dec, streams, tmp_path):
    damaged = ref.damaged_set()
    # first on the host, the same header: a damaged stream reaches the device only after the host program ended it with its status
    exe = ref.compile_inflate_program(tmp_path)
    host = ref.run_inflate_program(exe, [(s, cap) for _, s, cap, _ in damaged])
    assert [h[0] for h in host] == [bit for _, _, _, bit in damaged] and all(h[2] and h[1] <= cap for h, (_, _, cap, _) in zip(host, damaged))
    good = [s for s in streams if len(s[2]) <= 9000]
    mixed, caps = [], []
    for k, (name, s, cap, bit) in enumerate(damaged):
        g = good[k % len(good)]
        mixed += [s, g[1]]
        caps += [cap, len(g[2])]
    outs, lengths, status = dec.inflate_streams(mixed, caps)
    for k, (name, s, cap, bit) in enumerate(damaged):
        assert int(status[2 * k]) == bit, (name, int(status[2 * k]), bit)
        assert int(lengths[2 * k]) == host[k][1] and outs[2 * k].cpu().numpy().tobytes() == host[k][3], name
        g = good[k % len(good)]
        assert int(status[2 * k + 1]) == 0 and outs[2 * k + 1].cpu().numpy().tobytes() == g[2], name


def test_a_damaged_stream_writes_nothing_behind_its_capacity(dec):
    import torch
    from sniper_amd import hip
    # the entry point itself, with a guard behind every output
    damaged = [d for d in ref.damaged_set() if d[3] == 128]
    S = len(damaged)
    data = np.frombuffer(b''.join(s for _, s, _, _ in damaged), np.uint8)
    tab = np.zeros((S, 4), np.int64)
    tab[:, 1] = [len(s) for _, s, _, _ in damaged]
    tab[:, 0] = np.concatenate([[0], np.cumsum(tab[:, 1])[:-1]])
    tab[:, 3] = [cap for _, _, cap, _ in damaged]
    tab[:, 2] = np.concatenate([[0], np.cumsum(tab[:, 3] + 64)[:-1]])
    total = int((tab[:, 3] + 64).sum())
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device='cuda')
    meta = torch.zeros((S, 2), dtype=torch.int32, device='cuda')
    hip.call('sn_inflate', hip.dev(data.copy()), data.size, hip.dev(tab), tab, S, out, total, meta, hip.stream())
    h_out, h_meta = out.cpu().numpy(), meta.cpu().numpy()
    for k in range(S):
        assert h_meta[k, 1] == 128 and h_meta[k, 0] <= tab[k, 3]
        assert (h_out[tab[k, 2] + tab[k, 3]:tab[k, 2] + tab[k, 3] + 64] == 0xA5).all(), damaged[k][0]


# ---- PNG -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files():
    front = ref.matrix_files(sizes=ref.FRONT_SIZES, combos=((2, 8), (3, 4), (6, 16), (0, 1)), seed=21)
    return ref.matrix_files() + ref.special_files() + front


def test_decode_equals_pil_on_the_matrix_in_one_mixed_batch(dec, files, tmp_path):
    want = [ref.pil_bgr(d) for _, d in files]
    sources = []
    for k, (name, d) in enumerate(files):          # paths and bytes, mixed
        if k % 7 == 0:
            path = str(tmp_path / (name + '.png'))
            with open(path, 'wb') as fh:
                fh.write(d)
            sources.append(path)
        else:
            sources.append(d)
    dec.reset_stats()
    got = dec.decode_png(sources)
    assert dec.stats() == {'device': len(files), 'fallback': {}}
    for (name, _), g, w in zip(files, got, want):
        assert g.is_cuda and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), name
        assert g.untyped_storage().nbytes() == g.numel()
    # the 64-lane front's edges are in the batch
    sizes = {w.shape[:2] for w in want}
    assert {h for h, _ in sizes} >= {63, 64, 65, 129} and {w for _, w in sizes} >= {1, 2, 63, 64, 65}


def test_index_mode_equals_getdata_for_palette_and_grey_files(dec, files):
    idx = [(n, d) for n, d in files if ref.read_png(d)['ctype'] in (0, 3)]
    assert len(idx) > 100
    dec.reset_stats()
    got = dec.decode_png([d for _, d in idx], mode='index')
    assert dec.stats() == {'device': len(idx), 'fallback': {}}
    for (name, d), g in zip(idx, got):
        w = ref.pil_index(d)
        assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), name
    # an RGB file in index mode is the parent's: np.array(getdata(), uint8) of tuples cannot be reshaped to (h, w)
    rgb = [d for n, d in files if n.startswith('c2_d8_9x13')][0]
    with pytest.raises(ValueError):
        dec.decode_png([rgb], mode='index')
    assert dec.stats()['fallback'] == {'not_indexed': 1}


def test_round_trip_through_the_device_encoder(dec):
    from sniper_amd import png
    rng = np.random.default_rng(3)
    pics = [rng.integers(0, 256, (37, 53, 3)).astype(np.uint8),
            np.full((70, 600, 3), 9, np.uint8),                                   # runs: matches at distance 1, one distance code
            (np.cumsum(rng.integers(-3, 4, (129, 65, 3)), axis=1) + 100).astype(np.uint8),
            np.zeros((1, 1, 3), np.uint8)]
    big = np.zeros((64, 400, 3), np.uint8)                                       # more than one 32 KiB block: empty stored blocks between
    big[:, :, 0] = np.arange(400) // 7
    big[:, :, 1:] = rng.integers(0, 3, (64, 400, 2))
    pics.append(big)
    data = png.encode_png(pics)
    dec.reset_stats()
    got = dec.decode_png(data)
    assert dec.stats() == {'device': len(pics), 'fallback': {}}
    for p, g in zip(pics, got):
        assert np.array_equal(g.cpu().numpy()[:, :, ::-1], p)


def test_fallbacks_give_the_parents_pixels_or_its_exception(dec, tmp_path):
    from sniper_amd.data.im_worker import load_bgr
    rng = np.random.default_rng(4)
    pix = rng.integers(0, 256, (19, 23, 3)).astype(np.uint8)
    laced = ref.adam7_png_bytes(pix, 2)
    assert np.array_equal(ref.pil_bgr(laced)[:, :, ::-1], pix)
    g16 = ref.png_bytes(11, 5, 16, 0, rng.integers(0, 256, (5, 22)).astype(np.uint8), [0, 1, 2, 3, 4])
    plain = ref.png_bytes(23, 19, 8, 2, pix.reshape(19, -1), [4] * 19)
    dec.reset_stats()
    got = dec.decode_png([laced, plain, g16])
    assert dec.stats() == {'device': 1, 'fallback': {'interlaced': 1, 'gray16': 1}}
    for d, g in zip((laced, plain, g16), got):
        assert np.array_equal(g.cpu().numpy(), load_bgr(io.BytesIO(d)))
    # a wrong Adler-32 (every chunk CRC right): PIL raises, and so does decode_png -- after the device said why
    raw = ref.filter_rows(pix.reshape(19, -1), [1] * 19, 3)
    z = zlib.compress(raw)
    bad = ref.png_bytes(23, 19, 8, 2, zdata=z[:-1] + bytes([z[-1] ^ 0x55]))
    with pytest.raises(Exception) as parent:
        load_bgr(io.BytesIO(bad))
    dec.reset_stats()
    with pytest.raises(type(parent.value)):
        dec.decode_png([plain, bad])
    assert dec.stats() == {'device': 1, 'fallback': {'damaged_adler': 1}}
    # a filter type above 4, and a stream one row short: flagged, then the parent's
    for name, zdata in (('damaged_filter_type', zlib.compress(b'\x07' + raw[1:])), ('damaged_raw_length', zlib.compress(raw[:-70]))):
        f = ref.png_bytes(23, 19, 8, 2, zdata=zdata)
        dec.reset_stats()
        try:
            want = load_bgr(io.BytesIO(f))
        except Exception as e:          # noqa: BLE001
            with pytest.raises(type(e)):
                dec.decode_png([f])
        else:
            assert np.array_equal(dec.decode_png([f])[0].cpu().numpy(), want)
        assert dec.stats() == {'device': 0, 'fallback': {name: 1}}


def test_the_image_cache_decodes_png_paths_on_the_device(dec, tmp_path, monkeypatch):
    import torch
    from sniper_amd.data import im_worker as iw
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    rng = np.random.default_rng(6)
    paths = []
    for k, (h, w) in enumerate(((40, 60), (33, 21), (64, 64))):
        rows = ref.random_rows(rng, h, w, 8, 2, smooth=True)
        p = str(tmp_path / ('im%d%s' % (k, '.PNG' if k == 1 else '.png')))
        with open(p, 'wb') as fh:
            fh.write(ref.png_bytes(w, h, 8, 2, rows, [(y + k) % 5 for y in range(h)]))
        paths.append(p)
    calls = []
    real = dec.decode_png
    monkeypatch.setattr(dec, 'decode_png', lambda srcs, *a, **k: calls.append(len(srcs)) or real(srcs, *a, **k))
    pil, device = iw.DeviceImageCache(decoder='pil'), iw.DeviceImageCache(decoder='device')
    a = pil.get_many(paths)
    assert calls == []
    b = device.get_many(paths + [paths[0]])
    assert calls == [3] and device.misses == 3          # one batched call
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(b[3], a[0])
    other = iw.DeviceImageCache(decoder='device')
    assert torch.equal(other.get(paths[1]), a[1]) and calls == [3, 1]
    assert iw.DeviceImageCache().decoder == 'pil'


# ---- the VOC ground truth ---------------------------------------------------------------------------------------------------------
def _same_records(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g['mask'].dtype == np.bool_ and g['mask'].shape == w['mask'].shape and np.array_equal(g['mask'], w['mask'])
        assert np.array_equal(g['mask_bound'], w['mask_bound']) and np.asarray(g['mask_bound']).dtype.kind == 'i'
        assert int(g['mask_cls']) == int(w['mask_cls'])


def test_voc_instances_equal_the_restatement():
    import torch
    from sniper_amd import voc_gt
    maps = ref.voc_maps()
    got = voc_gt.voc_instances([torch.from_numpy(o).cuda() for o, _ in maps], [torch.from_numpy(c).cuda() for _, c in maps])
    assert len(got) == len(maps)
    for (o, c), g in zip(maps, got):
        _same_records(g, ref.parse_inst_ref(o, c))
    assert [int(r['mask_cls']) for r in got[0]] == [255] and got[0][0]['mask_bound'].tolist() == [0, 0, 0, 0]
    ids = [1, 2, 3, 7, 9, 255]
    assert len(got[1]) == len(ids) and got[1][2]['mask_bound'].tolist() == [0, 0, 52, 36] and got[1][3]['mask'].shape == (1, 1)
    # an image without instances, between two with
    empty = np.zeros((4, 5), np.uint8)
    got = voc_gt.voc_instances([maps[1][0], empty, maps[0][0]], [maps[1][1], empty, maps[0][1]])
    assert got[1] == [] and len(got[0]) == len(ids) and len(got[2]) == 1


def test_voc_instances_refuse_what_the_reference_refuses():
    from sniper_amd import voc_gt
    obj, cls = [m.copy() for m in ref.voc_maps()[1]]
    cls[6, 10] = 3                                     # instance 2 now carries two classes
    with pytest.raises(AssertionError) as e:
        ref.parse_inst_ref(obj, cls)
    with pytest.raises(AssertionError) as e:
        voc_gt.voc_instances([obj, obj], [ref.voc_maps()[1][1], cls], names=['a', 'b'])
    assert "'b'" in str(e.value) and 'instance 2' in str(e.value)
    with pytest.raises(ValueError):
        voc_gt.voc_instances([obj], [cls[:-1]])
    with pytest.raises(ValueError):
        voc_gt.voc_instances([obj, obj], [cls])


def test_parse_inst_batch_feeds_the_mask_evaluator(tmp_path):
    from sniper_amd import voc_gt
    from sniper_amd.evaluation import VOCSegmEvaluator
    rng = np.random.default_rng(8)
    maps = ref.voc_maps()[1:]
    names = ['2008_000001', '2008_000002']
    for sub in ('SegmentationObject', 'SegmentationClass'):
        os.makedirs(str(tmp_path / sub))
    pal = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    for name, (obj, cls) in zip(names, maps):
        cls = np.where(cls == 255, 0, cls).astype(np.uint8)          # (classes 1 .. 20 for the evaluator; the void label is not an instance's)
        obj = np.where(obj == 255, 0, obj).astype(np.uint8)
        for sub, m in (('SegmentationObject', obj), ('SegmentationClass', cls)):
            h, w = m.shape
            with open(str(tmp_path / sub / (name + '.png')), 'wb') as fh:
                fh.write(ref.png_bytes(w, h, 8, 3, m, [(y * 2) % 5 for y in range(h)], palette=pal))
    records = voc_gt.parse_inst_batch(names, str(tmp_path))
    for name, rec in zip(names, records):
        o = ref.pil_index(open(str(tmp_path / 'SegmentationObject' / (name + '.png')), 'rb').read())
        c = ref.pil_index(open(str(tmp_path / 'SegmentationClass' / (name + '.png')), 'rb').read())
        _same_records(rec, ref.parse_inst_ref(o, c))
    ev = VOCSegmEvaluator(records, 2, ['__background__'] + ['c%d' % k for k in range(1, 21)])
    assert len(ev.gt['image']) == sum(len(r) for r in records) == 10
