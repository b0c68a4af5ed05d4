"""CPU: pin the oracle (oracle/dbde_oracle.c) to the reference.

Three anchors, strongest first:
  1. the reference's own known-answer vector (dbde_util_test.cpp:135-178),
  2. tests/golden/ fixtures produced by the real reference (make_golden.py),
  3. a differential run of random frames against the reference's recorded results (tests/golden/reference_runs.json),
     and live against oracle/_ref/libdbde_ref.so when it is present.
"""
import hashlib

import numpy as np
import pytest
from oracle_ffi import Reference, differential_cases, reference_runs, wrapping_add_stream

MODES = {"noise8": 0, "mixed": 1, "flat": 2, "smooth": 3}

# dbde_util_test.cpp:145-178 -- the reference's asserted 128-byte stream for the 8x16 image
KAT_STREAM = bytes([
    3, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 240, 63,
    2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    2, 0, 0, 0, 4, 4, 2, 0, 0, 0, 0, 8, 8, 0, 0, 0,
    0x10, 0x39, 0x54, 0x76, 0x38, 0x54, 0x76, 0x98, 0x54, 0x76, 0x98, 0xBA, 0x76, 0x98, 0xBA, 0xDC,
    0x87, 0xA9, 0xCB, 0xED, 0x65, 0x87, 0xA9, 0xCB, 0x43, 0x65, 0x87, 0xA9, 0x21, 0x43, 0x65, 0x87,
    0x10, 0x32, 0x54, 0x76, 0x32, 0x54, 0x76, 0x98, 0x54, 0x76, 0x98, 0xBA, 0x76, 0x98, 0xBA, 0xDC,
    0x87, 0xA9, 0xCB, 0xED, 0x65, 0x87, 0xA9, 0xDB, 0x43, 0x65, 0x87, 0xCA, 0x21, 0x43, 0x75, 0xB9])

# reference output for the README 10x10 frame, index 7 (trap T2: the last
# three words differ from the README's printed ones)
README_WORDS = [0x298362534A53A486, 0x630926404916A376, 0x657A9CBC78469B68, 0x36AADCCA89896D9B,
                0xFFFD5556AAAB0001, 0x5554AAAAAAAB0000, 0x5FF6045FF600A773, 0xF6045FF6045FF604,
                0x045FF6045FF6045F]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_reference_known_answer_vector(oracle, golden):
    _, arrays = golden
    img = arrays["kat_8x16.image"]
    stream = np.frombuffer(KAT_STREAM, np.uint8)
    assert len(stream) == 128
    # unpack side (dbde_util_test.cpp:187-198)
    n, vh = oracle.unpack_video_header(stream)
    assert n == 28 and vh == (3, 8, 16, 1.0)
    n, fh = oracle.unpack_frame_header(stream[28:])
    assert n == 20 and fh == (2, 1, 0)
    n, fh, back = oracle.unpack_frame(stream[28:], 16, 8)
    assert n == 100 and fh == (2, 1, 0) and (back == img).all()
    # pack side (:199-212)
    out = np.concatenate([oracle.pack_video_header(3, 8, 16, 1.0), oracle.pack_frame(1, img, 16, 8)])
    assert out.tobytes() == KAT_STREAM


def test_readme_example(oracle, golden):
    _, arrays = golden
    packed = oracle.pack_frame(7, arrays["readme_10x10.image"], 10, 10)
    assert len(packed) == 112
    assert packed[:20].tobytes() == bytes([2, 0, 0, 0, 7] + [0] * 15)
    assert packed[20:40].tobytes() == bytes([4, 0, 0, 0, 4, 2, 3, 0, 4, 0, 0, 0, 0x13, 0x18, 0x1C, 0x1A, 9, 0, 0, 0])
    assert packed[40:].view("<u8").tolist() == README_WORDS


def test_all_golden_frames(oracle, golden):
    manifest, arrays = golden
    assert len(manifest["frames"]) >= 50
    for e in manifest["frames"]:
        img, want = arrays[e["name"] + ".image"], arrays[e["name"] + ".packed"]
        got = oracle.pack_frame(e["index"], img, e["W"], e["H"])
        assert got.tobytes() == want.tobytes(), e["name"]
        n, fh, back = oracle.unpack_frame(want, e["W"], e["H"])
        assert n == len(want) and fh == (2, e["index"], 0) and (back == img).all(), e["name"]


def test_synth_inputs_are_the_golden_inputs(oracle, golden):
    manifest, arrays = golden
    for e in manifest["frames"]:
        if not e["name"].startswith("synth_"):
            continue
        mode = MODES[e["name"].split("_")[1]]
        img = oracle.synth_frame(mode, manifest["seed"], e["index"], e["W"], e["H"])
        assert (img == arrays[e["name"] + ".image"]).all(), e["name"]


def test_tile_demos_and_depth_bounds(oracle, golden):
    manifest, arrays = golden
    flat = arrays["demo_10x10.image"].reshape(-1)
    for t in manifest["tile_demos"]:
        if t["rm"] == 8 and t["dm"] == 8:
            code, payload, raw = oracle.pack_8x8(flat, t["off"], 10)
        else:
            code, payload, raw = oracle.pack_8x8_partial(flat, t["off"], 10, t["rm"], t["dm"])
        assert code == t["code"] and payload.tobytes().hex() == t["payload"]
        assert (raw[len(payload):] == 0xEE).all()          # writes exactly 8*depth bytes
        # decode back into a strided canvas, partial writes only the valid region
        canvas = np.full(100, 0xEE, np.uint8)
        oracle.unpack_8x8_partial(code >> 8, code & 0xFF, payload, 10, t["rm"], t["dm"], canvas, 0)
        got = canvas.reshape(10, 10)
        src = flat.reshape(10, 10)
        y0, x0 = divmod(t["off"], 10)
        assert (got[:t["dm"], :t["rm"]] == src[y0:y0 + t["dm"], x0:x0 + t["rm"]]).all()
        got[:t["dm"], :t["rm"]] = 0xEE
        assert (got == 0xEE).all()
    for rng, depth in manifest["depth_bounds"]:
        tile = np.zeros(64, np.uint8)
        tile[5] = rng
        code, payload, _ = oracle.pack_8x8(tile, 0, 8)
        assert code >> 8 == depth and len(payload) == 8 * depth


def test_headers(oracle, golden):
    manifest, _ = golden
    for h in manifest["headers"]["frame"]:
        wire = oracle.pack_frame_header(*h["in"])
        assert wire.tobytes().hex() == h["wire"]
        n, out = oracle.unpack_frame_header(wire)
        assert n == h["advance"] and list(out) == h["out"]
    for h in manifest["headers"]["video"]:
        wire = oracle.pack_video_header(*h["in"])
        assert wire.tobytes().hex() == h["wire"]
        n, out = oracle.unpack_video_header(wire)
        assert n == h["advance"] and list(out) == h["out"]


def test_malformed(oracle, golden):
    manifest, arrays = golden
    base = arrays["malformed_base.packed"]
    for m in manifest["malformed"]:
        bad = base.copy()
        bad[m["pos"]] = (int(bad[m["pos"]]) + m["delta"]) % 256
        n, fh, img = oracle.unpack_frame(bad, 10, 10, fill=0xEE)
        assert n == m["advance"] and fh[0] == m["u64s"] and fh[1] == m["index"], m["label"]
        assert bool((img == 0xEE).all()) == m["image_untouched"] and sha(img) == m["image_sha"]
        n_img, _ = oracle.unpack_image(bad[20:], 10, 10)
        assert n_img == m["unpack_image_ret"]
    # the one intentional deviation: depth byte > 8 is rejected (reference: unchecked, trap T8)
    bad = base.copy()
    bad[24] = 9
    bad[36] = (int(bad[36]) + 5) % 256          # keep n64 == sum(depth) so only the depth check trips
    n, fh, img = oracle.unpack_frame(bad, 10, 10, fill=0xEE)
    assert n == 20 and fh[0] == 0xFFFFFFFF and (img == 0xEE).all()


def test_big_config_hashes(oracle, golden):
    """BASELINE.json configs 2-4 at full size: oracle output hashes == reference output hashes."""
    manifest, _ = golden
    for e in manifest["big"]:
        if e["frame"] not in (0, 1024) and e["name"].startswith("cfg2"):
            continue  # keep the CPU suite short; the other frames are covered by the GPU parity tests
        img = oracle.synth_frame(MODES[e["mode"]], manifest["seed"], e["frame"], e["W"], e["H"])
        assert sha(img) == e["image_sha"]
        packed = oracle.pack_frame(e["frame"], img, e["W"], e["H"])
        assert len(packed) == e["packed_bytes"] and sha(packed) == e["packed_sha"], e
        T = ((e["W"] + 7) // 8) * ((e["H"] + 7) // 8)
        assert np.bincount(packed[24:24 + T], minlength=9).tolist() == e["depth_hist"]
        n, fh, back = oracle.unpack_frame(packed, e["W"], e["H"])
        assert n == len(packed) and (back == img).all()


def test_live_differential_against_reference(oracle):
    """300 random frames: the oracle's packed bytes and unpack against the reference's, as recorded by make_golden.py
    (tests/golden/reference_runs.json) and, where oracle/_ref is built, against the live reference as well."""
    runs = reference_runs()
    reference = Reference() if Reference.available() else None
    cases = list(differential_cases(oracle))
    assert len(cases) == len(runs["differential"])
    for (W, H, kind, img, idx), want in zip(cases, runs["differential"]):
        assert (W, H, kind, idx, sha(img)) == (want["W"], want["H"], want["kind"], want["index"], want["image_sha"])
        a = oracle.pack_frame(idx, img, W, H)
        assert len(a) == want["packed_bytes"] and sha(a) == want["packed_sha"], (W, H, kind)
        na, fa, ia = oracle.unpack_frame(a, W, H)
        assert na == want["advance"] == len(a) and list(fa) == want["header"] and sha(ia) == want["unpacked_sha"]
        assert (ia == img).all()
        if reference is not None:
            b = reference.pack_frame(idx, img, W, H)
            assert a.tobytes() == b.tobytes(), (W, H, kind)
            nb, fb, ib = reference.unpack_frame(a, W, H)
            assert na == nb and fa == fb and (ia == ib).all()
    # byte-wise wrapping add on decode (min + value > 255 in a crafted but accepted stream)
    packed = wrapping_add_stream(oracle)
    want = runs["wrapping_add"]
    assert packed.tobytes().hex() == want["stream"]
    na, fa, ia = oracle.unpack_frame(packed, 8, 8)
    assert na == want["advance"] and list(fa) == want["header"] and ia.tobytes().hex() == want["image"]
    assert ia[0, 1] == (255 + 200) % 256
    if reference is not None:
        nb, fb, ib = reference.unpack_frame(packed, 8, 8)
        assert na == nb and fa == fb and (ia == ib).all()
