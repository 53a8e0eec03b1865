"""Legacy (magic 0 / 1) MessageSets -> v2 batches on the device
(rpgpu_legacy_plan_device / rpgpu_legacy_run_device, rpgpu_crc32_ranges_device
and the scalar mirrors), compared byte for byte with the restatement
tests/legacy_sets.py: the result row, the whole rewritten batch, d_out_results
against the oracle's validation of the expected batch, and the index."""
import struct
import zlib

import numpy as np
import pytest

import kafka_batches as kb
import legacy_sets as ls
import oracle.oracle as orc

pytestmark = pytest.mark.gpu

NOW = 1_700_000_123_456
LENS = (None, 0, 1, 15, 16, 17, 63, 64, 8191, 8192)


def compare(eng, sets, align=None, expected=None):
    """Convert `sets` (bytes, or None for a null-records descriptor) on the
    device and check everything against the restatement."""
    from redpanda_amd import abi

    data, descs = ls.arena(sets, align)
    got = eng.convert_legacy_sets(data, descs, NOW)
    lres = got["lres"]
    want = expected if expected is not None else [None if s is None else ls.convert(s, NOW) for s in sets]
    exp_data = np.zeros(len(got["out"]), dtype=np.uint8)
    exp_descs = np.zeros(len(sets), dtype=orc.DESC_DTYPE)
    exp_descs["partition"] = descs["partition"]
    exp_descs["format"] = kb.DISK
    nrec = 0
    for i, w in enumerate(want):
        r = lres[i]
        if w is None:
            assert (r["verdict"], r["event_message"], r["codec"]) == (abi.V_NULL_RECORDS, -1, 0), i
            continue
        v, ev, codec, batch = w
        assert (int(r["verdict"]), int(r["event_message"]), int(r["codec"])) == (v, ev, codec), \
            (i, r, (v, ev, codec))
        if v != ls.V_OK:
            continue
        a, m = int(r["out_offset"]), int(r["out_len"])
        assert m == len(batch) and m <= int(r["out_cap"]) and a + m <= got["out_bytes"], i
        assert got["out"][a:a + m].tobytes() == batch, f"rewritten batch {i} differs"
        n = struct.unpack_from("<i", batch, 57)[0]
        assert int(r["record_count"]) == n and int(r["timestamp"]) == struct.unpack_from("<q", batch, 27)[0], i
        exp_data[a:a + m] = np.frombuffer(batch, dtype=np.uint8)
        exp_descs["offset"][i], exp_descs["length"][i], exp_descs["ops"][i] = a, m, 15
        nrec += n
    od = got["out_descs"]
    for f in ("offset", "length", "partition", "format"):
        assert np.array_equal(od[f], exp_descs[f]), f
    assert ((od["ops"] != 0) == (exp_descs["length"] != 0)).all()
    assert nrec <= got["records_total"]
    wres, windex, wused = orc.validate_arena(exp_data, exp_descs)
    for f in abi.RESULT_DTYPE.names:
        bad = np.nonzero(got["out_results"][f] != wres[f])[0]
        assert bad.size == 0, f"out_results field {f} differs at {bad[:8]}: {got['out_results'][f][bad[:8]]} vs {wres[f][bad[:8]]}"
    assert got["used"] == wused
    assert np.array_equal(got["index"].view(np.uint8), windex[:wused].view(np.uint8)), "index differs"
    return got, want


@pytest.mark.parametrize("with_seed", [True, False])
def test_crc32_ranges_device(eng, with_seed):
    import torch

    rng = np.random.default_rng(21 + with_seed)
    big = (1 << 20) + 3
    data = rng.integers(0, 256, big + 16 + 64, dtype=np.uint8)
    lens_one = list(range(0, 81)) + [1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, big]
    offs = np.array([a for a in range(16) for _ in lens_one], dtype=np.uint64)
    lens = np.array([l for _ in range(16) for l in lens_one], dtype=np.uint32)
    n = len(lens)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dev = torch.device("cuda", 0)
    d_data = torch.from_numpy(data).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_seed = torch.from_numpy(seeds.view(np.int32)).to(dev) if with_seed else None
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    eng.crc32_ranges_device(d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                            d_seed.data_ptr() if with_seed else 0, n, d_out.data_ptr(), sh)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    raw = data.tobytes()
    for i in range(n):
        o, l = int(offs[i]), int(lens[i])
        want = zlib.crc32(raw[o:o + l], int(seeds[i]) if with_seed else 0)
        assert int(got[i]) == want, (o, l)


def test_crc32_extend_mirror(eng):
    rng = np.random.default_rng(5)
    assert eng.crc32_extend(0, b"123456789") == 0xCBF43926
    assert eng.crc32_extend(0, b"") == 0
    for n in (1, 3, 4, 17, 1024, 70001):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert eng.crc32_extend(0, b) == zlib.crc32(b), n
        half = n // 2                                     # chained in two halves
        assert eng.crc32_extend(eng.crc32_extend(0, b[:half]), b[half:]) == zlib.crc32(b), n


def _geometry_sets():
    rng = np.random.default_rng(33)
    sets, k = [], 0

    def payload(l):
        return None if l is None else rng.integers(0, 256, l, dtype=np.uint8).tobytes()

    for count in (0, 1, 2, 63, 64, 65, 129):
        for mode in ("magic0", "magic1", "mixed_last0"):
            msgs = []
            for j in range(count):
                kl, vl = LENS[k % 10], LENS[(k // 10) % 10]
                k += 1
                magic = {"magic0": 0, "magic1": 1}.get(mode, 0 if j == count - 1 else int(rng.integers(0, 2)))
                if mode == "mixed_last0" and j == 0 and count > 1:
                    magic = 1
                msgs.append(dict(key=payload(kl), value=payload(vl), magic=magic, ts=int(rng.integers(1, 1 << 41))))
            sets.append(ls.message_set(msgs))
    small = (None, 0, 1, 15, 16, 17)
    sets.append(ls.message_set([dict(key=payload(small[j % 6]), value=payload(small[(j // 6) % 6]), magic=j & 1,
                                     ts=1_650_000_000_000 + j) for j in range(8193)]))
    sets.append(ls.message_set([dict(key=b"big", value=payload(1 << 20), magic=1, ts=5),
                                dict(key=None, value=b"after", magic=0)]))
    sets.append(None)                                      # a null-records descriptor
    for a in range(16):                                    # every start alignment
        sets.append(ls.message_set([dict(key=payload(17), value=payload(100 + a), magic=1, ts=77 + a),
                                    dict(key=None, value=payload(300), magic=0),
                                    dict(key=payload(1), value=None, magic=1, ts=99 + a)]))
    align = [(3 * i) % 16 for i in range(len(sets) - 16)] + list(range(16))
    return sets, align


def test_geometry(eng):
    sets, align = _geometry_sets()
    got, want = compare(eng, sets, align)
    assert all(w is None or w[0] == ls.V_OK for w in want)
    counts = [struct.unpack_from("<i", w[3], 57)[0] for w in want if w is not None]
    assert {0, 1, 2, 63, 64, 65, 129, 8193} <= set(counts)
    # a plan may be run any number of times: the second run starts from fresh
    # event keys and work lists and leaves the same output
    data, descs = ls.arena(sets, align)
    again = eng.convert_legacy_sets(data, descs, NOW, runs=2)
    for f in ("lres", "out_descs", "out_results", "index"):
        assert np.array_equal(again[f].view(np.uint8), got[f].view(np.uint8)), f
    for r in got["lres"][got["lres"]["verdict"] == 0]:
        o, m = int(r["out_offset"]), int(r["out_len"])
        assert np.array_equal(again["out"][o:o + m], got["out"][o:o + m])


def _with_bad_crc(kw, following):
    good = ls.message(following=following, **kw)
    crc = struct.unpack_from(">I", good, 12)[0]
    return ls.message(following=following, crc=crc ^ 0x10, **kw)


def test_batch_length_corners(eng):
    """batch_length only sets the CRC range: true, 4, 3 / 0 / -1 (wrap: everything
    left), true + 1 and spanning the next message (over the following bytes),
    past the end (clamped); each with a CRC that matches the clamped range
    (the set converts) and with one that does not (CRC mismatch at message 1)."""
    first = dict(key=b"a", value=b"first", magic=1, ts=10, offset=0)
    last = ls.message(b"z", b"last message", magic=0, offset=2)
    mid = dict(key=b"mid", value=b"middle value", magic=1, ts=20, offset=1)
    true_len = len(ls.message(**mid)) - 12
    sets = []
    for bl in (None, 4, 3, 0, -1, true_len + 1, true_len + len(last), 1 << 30):
        kw = dict(mid, batch_length=bl)
        m_ok = ls.message(following=last, **kw)
        m_bad = _with_bad_crc(kw, last)
        head = ls.message(following=m_ok + last, **first)
        sets.append(head + m_ok + last)
        sets.append(ls.message(following=m_bad + last, **first) + m_bad + last)
    got, want = compare(eng, sets)
    assert [w[0] for w in want] == [ls.V_OK, ls.V_LEGACY_CRC_MISMATCH] * 8
    assert all(w[1] == 1 for w in want[1::2])


def _verdict_sets():
    good = [dict(key=b"k%d" % j, value=b"value-%d" % j * 3, magic=j & 1, ts=1000 + j) for j in range(8)]

    def flip_crc(msgs, j):
        out = [dict(m) for m in msgs]
        tail = ls.message_set(out[j + 1:]) if j + 1 < len(out) else b""
        kw = dict(out[j])
        kw.setdefault("offset", j)
        bad = _with_bad_crc(kw, tail)
        return ls.message_set(out[:j]) + bad + tail

    def edit(msgs, j, **kw):
        out = [dict(m) for m in msgs]
        out[j].update(kw)
        return out

    full = ls.message_set(good)
    upto5 = len(ls.message_set(good[:5]))
    named = {
        "ok": full,
        "magic": ls.message_set(edit(good, 2, magic=2)),
        "crc": flip_crc(good, 4),
        "lz4_magic0": ls.message_set(edit(good, 3, magic=0, attrs=3)),
        "null_compressed": ls.message_set(edit(good, 3, magic=1, attrs=1, value=None)),
        "trunc_header": full[:upto5 + 9],                 # stage before the CRC
        "trunc_value": full[:upto5 - 2],                  # message 4's value cut: CRC clamps, then fails first
        "bad_codec_4": ls.message_set(edit(good, 1, attrs=4)),
        "bad_codec_5": ls.message_set(edit(good, 1, attrs=5)),
        "bad_codec_6": ls.message_set(edit(good, 1, attrs=6)),
        "bad_codec_7": ls.message_set(edit(good, 1, attrs=7 | 8)),
        "wrapper_gzip": ls.message_set(edit(good, 6, attrs=1)),
        "wrapper_snappy": ls.message_set(edit(good, 6, attrs=2)),
        "wrapper_lz4": ls.message_set(edit(good, 7, magic=1, attrs=3)),
        # precedence
        "crc3_then_trunc5": flip_crc(good, 3)[:upto5 + 20],
        "trunc3_then_crc5": None,                         # filled below
        "magic_and_crc": flip_crc(edit(good, 2, magic=9), 2),
        "crc_and_trunc_value": None,
        "neg_key_size": None,
        "trail_1": full + b"\x00",
        "trail_11": full + b"\x00" * 11,
        "trail_15": full + b"\x07" * 15,
    }
    # a truncation at message 3 (its value size points past the set) before a CRC failure at 5:
    # the size field is covered by a fresh CRC, so the truncation is the first event
    m3 = dict(good[3])
    s = bytearray(ls.message_set(good[:4]))
    at = len(s) - 4 - len(m3["value"])
    struct.pack_into(">i", s, at, 1 << 28)
    body = bytes(s[len(ls.message_set(good[:3])) + 16:])
    struct.pack_into(">I", s, len(ls.message_set(good[:3])) + 12, zlib.crc32(body))
    named["trunc3_then_crc5"] = bytes(s) + flip_crc(good, 5)[len(ls.message_set(good[:4])):]
    # a wrong CRC and a truncated value on the same (last) message: the CRC is checked first
    named["crc_and_trunc_value"] = flip_crc(good, 7)[:-3]
    s = bytearray(full)
    at = len(ls.message_set(good[:2])) + 16 + 1 + 1       # message 2 is magic 0: key size right after attrs
    struct.pack_into(">i", s, at, -2)
    struct.pack_into(">I", s, len(ls.message_set(good[:2])) + 12,
                     zlib.crc32(bytes(s[len(ls.message_set(good[:2])) + 16:len(ls.message_set(good[:3]))])))
    named["neg_key_size"] = bytes(s)
    return named


WANT_VERDICTS = {
    "ok": (0, -1), "magic": (50, 2), "crc": (51, 4), "lz4_magic0": (52, 3), "null_compressed": (53, 3),
    "trunc_header": (54, 5), "trunc_value": (51, 4), "bad_codec_4": (55, 1), "bad_codec_5": (55, 1),
    "bad_codec_6": (55, 1), "bad_codec_7": (55, 1), "wrapper_gzip": (56, 6), "wrapper_snappy": (56, 6),
    "wrapper_lz4": (56, 7), "crc3_then_trunc5": (51, 3), "trunc3_then_crc5": (54, 3), "magic_and_crc": (50, 2),
    "crc_and_trunc_value": (51, 7), "neg_key_size": (54, 2), "trail_1": (54, 8), "trail_11": (54, 8),
    "trail_15": (54, 8),
}


def test_verdicts_stages_and_precedence(eng):
    named = _verdict_sets()
    names = sorted(named)
    got, want = compare(eng, [named[k] for k in names])
    assert {k: (w[0], w[1]) for k, w in zip(names, want)} == WANT_VERDICTS
    codecs = {k: int(r["codec"]) for k, r in zip(names, got["lres"])}
    assert (codecs["wrapper_gzip"], codecs["wrapper_snappy"], codecs["wrapper_lz4"]) == (1, 2, 3)
    # run twice on one plan: the CRC events of the first run do not leak into the second
    data, descs = ls.arena([named[k] for k in names])
    again = eng.convert_legacy_sets(data, descs, NOW, runs=2)
    assert np.array_equal(again["lres"].view(np.uint8), got["lres"].view(np.uint8))


@pytest.fixture(scope="module")
def mutation():
    sets = ls.mutation_corpus(0x1E6AC7, 4000)
    return sets, [ls.convert(s, NOW) for s in sets]


def test_mutation_arena(eng, mutation):
    sets, want = mutation
    hist = {}
    for w in want:
        hist[w[0]] = hist.get(w[0], 0) + 1
    for v in (ls.V_OK,) + ls.LEGACY_VERDICTS:
        assert hist.get(v, 0) >= 20, (v, hist)
    assert hist[ls.V_OK] <= len(sets) // 2, hist
    compare(eng, sets, align=[(5 * i) % 16 for i in range(len(sets))], expected=want)


def test_chaining_submit_compress_decompress(eng, mutation):
    """The converted batches feed the rest of the engine unchanged."""
    from redpanda_amd import abi

    sets = [s for s, w in zip(*mutation) if w[0] == ls.V_OK][:200]
    data, descs = ls.arena(sets)
    got = eng.convert_legacy_sets(data, descs, NOW)
    assert (got["lres"]["verdict"] == 0).all()
    od = got["out_descs"].copy()
    od["ops"] = abi.OPS_PRODUCE
    res, index, used = eng.submit(got["out"], od)
    assert (res["verdict"] == abi.V_OK).all()
    assert np.array_equal(res["crc"], res["crc_expected"]) and np.array_equal(res["crc"], got["out_results"]["crc"])
    assert np.array_equal(res["header_crc"], got["out_results"]["header_crc"])
    comp = eng.compress_arena(got["out"], od, codec=3)
    assert (comp["cres"]["verdict"] == abi.V_OK).all()
    cd = comp["out_descs"].copy()
    cd["ops"] = abi.OPS_PRODUCE | abi.OP_DECOMP
    back = eng.decompress_arena(comp["out"], cd)
    nonempty = got["lres"]["record_count"] > 0                # an empty batch has no body to compress
    assert (back["dres"]["verdict"][nonempty] == abi.V_OK).all()
    for i in np.nonzero(nonempty)[0]:
        a, m = int(got["lres"]["out_offset"][i]), int(got["lres"]["out_len"][i])
        b, k = int(back["dres"]["out_offset"][i]), int(back["dres"]["out_len"][i])
        assert got["out"][a + 61:a + m].tobytes() == back["out"][b + 61:b + 61 + k].tobytes(), i


def test_scalar_mirror(eng):
    from test_legacy_sets import HAND_A, HAND_B, HAND_BODY

    v, batch, n = eng.convert_message_set(HAND_A + HAND_B, NOW)
    assert v == 0 and n == len(batch) == 61 + len(HAND_BODY) and batch[61:] == HAND_BODY
    assert batch == ls.convert(HAND_A + HAND_B, NOW)[3]
    named = _verdict_sets()
    for k in sorted(named):
        v, batch, n = eng.convert_message_set(named[k], NOW)
        w = ls.convert(named[k], NOW)
        assert v == w[0] == WANT_VERDICTS[k][0], k
        assert batch == w[3], k
    v, batch, n = eng.convert_message_set(b"", NOW)
    assert v == 0 and batch == ls.convert(b"", NOW)[3]
    v, batch, n = eng.convert_message_set(HAND_A + HAND_B, NOW, cap=70)    # too small: the size needed
    assert v == 34 and n == 61 + len(HAND_BODY)
