"""The REST proxy's fetch reply on the device (rpgpu_pp_fetch_plan_device /
rpgpu_pp_fetch_run_device) against the Python model tests/pp_fetch.py: the
sweep of the CPU half through eng.submit and eng.pp_fetch_json, bytes and
every result field; nothing outside the responses' own bytes is written (the
buffer is pre-filled with 0xA5); a plan run twice, a plan run once and a
second engine agree; small output buffers; rendering after decompression;
the reference's own vector; the format argument."""
import numpy as np
import pytest

import kafka_batches as kb
import pp_fetch as pp

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


@pytest.fixture(scope="module")
def eng2(built):
    from redpanda_amd import engine

    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sweeps():
    out = {}
    for fmt in (kb.WIRE, kb.DISK):
        case = pp.build_sweep(fmt)
        exp = case.expected()
        pp.assert_sweep_classes(case, exp)
        out[fmt] = (case, exp)
    return out


def validated(eng, case):
    data, descs = case.arena()
    res, index, _ = eng.submit(data, descs)
    return data, descs, res, index


def check(case, exp, out, got, out_cap=None):
    """Result rows and bytes against the model; everything else still FILL."""
    want, total = case.expected_results(exp, out_cap)
    for f in pp.RESULT_DTYPE.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{f} differs at {[case.names[i] for i in bad[:4]]}: {got[f][bad[:4]]} vs {want[f][bad[:4]]}"
    cap = total if out_cap is None else out_cap
    assert len(out) == cap + GUARD
    untouched = np.ones(len(out), dtype=bool)
    for i, e in enumerate(exp):
        if want["status"][i] != pp.OK:
            continue
        a, m = int(want["out_off"][i]), int(want["out_len"][i])
        assert a % 16 == 0 and a + m <= cap
        assert out[a:a + m].tobytes() == e[3], f"bytes of response {case.names[i]} differ"
        untouched[a:a + m] = False
    assert (out[untouched] == FILL).all(), f"written outside the responses at {np.nonzero(untouched & (out != FILL))[0][:8]}"
    return want, total


@pytest.mark.parametrize("fmt", [kb.WIRE, kb.DISK], ids=["wire", "disk"])
def test_sweep_parity(eng, sweeps, fmt):
    from redpanda_amd import abi

    case, exp = sweeps[fmt]
    assert abi.PP_LANE_FIELD_MAX == pp.LANE_FIELD_MAX
    # both paths carry keys and values
    for kv in (0, 1):
        lens = [ln for e in exp for k, ln, _ in e[4] if k == kv]
        assert any(ln <= abi.PP_LANE_FIELD_MAX for ln in lens) and any(ln > abi.PP_LANE_FIELD_MAX for ln in lens)
    data, descs, res, index = validated(eng, case)
    topics, ranges, responses = case.tables()
    out, got = eng.pp_fetch_json(data, descs, res, index, topics, ranges, responses, fill=FILL, guard=GUARD)
    want, _ = check(case, exp, out, got)
    assert set(want["status"]) == {pp.OK, pp.BAD_BATCH, pp.COMPRESSED, pp.NOT_INDEXED, pp.BAD_TOPIC, pp.BAD_RANGE}


def test_determinism(eng, eng2, sweeps):
    case, exp = sweeps[kb.DISK]
    data, descs, res, index = validated(eng, case)
    topics, ranges, responses = case.tables()
    args = (data, descs, res, index, topics, ranges, responses)
    a = eng.pp_fetch_json(*args, plans=2, runs=2, fill=FILL, guard=GUARD)
    b = eng.pp_fetch_json(*args, fill=FILL, guard=GUARD)
    c = eng2.pp_fetch_json(*args, fill=FILL, guard=GUARD)
    check(case, exp, *a)
    for o in (b, c):
        assert np.array_equal(a[0], o[0]) and np.array_equal(a[1].view(np.uint8), o[1].view(np.uint8))


def test_out_cap(eng):
    c = pp.Case(kb.DISK)
    for i in range(6):
        c.add(f"r{i}", [(b"cap", i, [pp.bspec([(pp.pattern(5 + 40 * i, i), pp.pattern(200 + i, i))], base=i)])]
              if i != 3 else [(b"bad topic", 0, [])])
    exp = c.expected()
    data, descs, res, index = validated(eng, c)
    topics, ranges, responses = c.tables()
    full, total = c.expected_results(exp)
    last = int(full["out_off"][5])
    assert total > last and total % 16 == 0
    mid = int(full["out_off"][2]) + int(full["out_len"][2]) // 2
    for cap, no_room in ((total, []), (total - 1, [5]), (mid, [2, 4, 5]), (0, [0, 1, 2, 4, 5])):
        out, got = eng.pp_fetch_json(data, descs, res, index, topics, ranges, responses, out_cap=cap, fill=FILL,
                                     guard=GUARD)
        want, _ = check(c, exp, out, got, out_cap=cap)          # earlier responses intact, nothing past out_cap
        assert list(np.nonzero(want["status"] == pp.NO_ROOM)[0]) == no_room, cap
        assert want["status"][3] == pp.BAD_TOPIC and (out[cap:] == FILL).all()


def test_after_decompression(eng):
    """gzip, snappy, LZ4 and zstd batches: rendered from the decompressor's
    output they give the original records; from the compressed arena,
    RPGPU_PP_COMPRESSED."""
    from redpanda_amd import abi

    c = pp.Case(kb.DISK)
    text = lambda i, m: (b"value %d of a compressible payload; " % i) * m        # noqa: E731
    c.add("decompressed", [(b"logs", 4, [pp.bspec([(b"k%d" % i, text(i, 1 + (i + j) % 9)) for i in range(1 + 20 * j)],
                                                  base=1000 * j) for j in range(4)]),
                           (b"metrics", 5, [pp.bspec([(None, text(7, 40)), (b"key", None)], base=77)])])
    exp = c.expected()
    data, descs = c.arena()
    topics, ranges, responses = c.tables()
    for codec in (1, 2, 3, 4):
        comp = eng.compress_arena(data, descs, codec)
        assert (comp["cres"]["verdict"] == 0).all() and (comp["out_results"]["codec"] == codec).all(), codec
        od = comp["out_descs"].copy()
        od["ops"] = abi.OPS_PRODUCE | abi.OP_DECOMP
        back = eng.decompress_arena(comp["out"], od)
        assert (back["dres"]["verdict"] == 0).all(), codec
        out, got = eng.pp_fetch_json(back["out"], back["out_descs"], back["out_results"], back["index"], topics,
                                     ranges, responses, fill=FILL, guard=GUARD)
        check(c, exp, out, got)
        out, got = eng.pp_fetch_json(comp["out"], od, back["results"], np.zeros(0, dtype=abi.INDEX_DTYPE), topics,
                                     ranges, responses, fill=FILL, guard=GUARD)
        assert len(got) == 1 and tuple(int(got[0][f]) for f in ("status", "bad_batch", "out_len", "records")) == \
            (pp.COMPRESSED, 0, 0, 0), codec
        assert (out == FILL).all()


@pytest.mark.parametrize("fmt", [kb.WIRE, kb.DISK], ids=["wire", "disk"])
def test_reference_vector(eng, fmt):
    case, want = pp.golden_case(fmt)
    exp = case.expected()
    assert [e[3] for e in exp] == want
    data, descs, res, index = validated(eng, case)
    topics, ranges, responses = case.tables()
    out, got = eng.pp_fetch_json(data, descs, res, index, topics, ranges, responses, fill=FILL, guard=GUARD)
    check(case, exp, out, got)


def test_format_argument(eng):
    from redpanda_amd import abi, engine

    case, _ = pp.golden_case(kb.DISK)
    exp = case.expected()
    data, descs, res, index = validated(eng, case)
    topics, ranges, responses = case.tables()
    args = (data, descs, res, index, topics, ranges, responses)
    none = eng.pp_fetch_json(*args, fmt=abi.PP_FMT_NONE, fill=FILL, guard=GUARD)
    v2 = eng.pp_fetch_json(*args, fmt=abi.PP_FMT_BINARY_V2, fill=FILL, guard=GUARD)
    check(case, exp, *v2)
    assert np.array_equal(none[0], v2[0]) and np.array_equal(none[1].view(np.uint8), v2[1].view(np.uint8))
    for fmt in (2, 8):                                   # json_v2 and anything unknown
        with pytest.raises(engine.EngineError, match=rf"rpgpu_pp_fetch_plan_device: {abi.RPGPU_EINVAL} "):
            eng.pp_fetch_json(*args, fmt=fmt)
