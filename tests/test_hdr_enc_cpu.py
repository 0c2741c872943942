"""The device Radiance HDR encoder's definition without a GPU: the segment rule as the kernels
compute it (tests/hdr_enc_ref.py: contributions and a prefix sum) equals the sequential loop of the reference's
writer (oracle.hdr_oracle._scanline) exhaustively over small alphabets, on random rows and on the crafted rows; the
crafted rows reach what they are for; the whole-file restatement equals the host library's encode_hdr; and the
argument checks of the native library need no device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import hdr_oracle
from tests import hdr_enc_cases as K
from tests import hdr_enc_ref as R


def _check_rows(rows: np.ndarray) -> None:
    coded, lens = R.code_rows(rows)
    ends = np.cumsum(lens)
    assert lens.max() <= R.row_bound(rows.shape[1])
    for i, row in enumerate(rows):
        assert coded[ends[i] - lens[i]:ends[i]].tobytes() == hdr_oracle._scanline(row.tobytes()), row.tolist()


@pytest.mark.parametrize("letters,lengths", [(2, range(8, 17)), (3, range(8, 11))])
def test_rule_equals_the_loop_exhaustively(letters, lengths):
    for n in lengths:
        digits = np.array(list(itertools.product(range(letters), repeat=n)), np.uint8)
        assert len(digits) == letters ** n
        _check_rows(digits * 7 + 1)


def test_rule_equals_the_loop_on_random_rows():
    rng = np.random.default_rng(5)
    done = 0
    for alphabet in (2, 4, 256):
        for _ in range(667):
            w = int(rng.integers(8, 701))
            _check_rows(rng.integers(0, alphabet, (1, w), dtype=np.uint8))
            done += 1
    assert done >= 2000


@pytest.mark.parametrize("name", sorted(K.rows()))
def test_crafted_rows(name):
    row, want = K.rows()[name]
    coded = R.code_row(row)
    assert coded == hdr_oracle._scanline(row.tobytes())
    assert R.tokens(coded) == want
    assert len(coded) <= R.row_bound(len(row))


def test_crafted_rows_reach_what_they_are_for():
    tok = {name: R.tokens(R.code_row(row)) for name, (row, _) in K.rows().items()}
    sizes = lambda name, kind: [t[1] for t in tok[name] if t[0] == kind]
    for w in (8, 126, 127, 128, 254, 255, 381):     # pieces of exactly 127, a remainder of 0 or 1
        assert sizes(f"constant_{w}", "run") == [127] * (w // 127) + ([w % 127] if w % 127 else [])
        assert not sizes(f"constant_{w}", "lit")
    assert {w % 127 for w in (127, 128, 254, 255, 381)} == {0, 1}
    for w in (128, 129, 256, 257):                  # dumps of exactly 128, a remainder of 1
        assert sizes(f"no_run_{w}", "lit") == [128] * (w // 128) + ([1] if w % 128 else [])
        assert not sizes(f"no_run_{w}", "run")
    assert tok["pairs"] == [("lit", 16)] and tok["pair_at_the_end"] == [("lit", 9)]
    assert sizes("run_of_3", "run") == [3]
    assert tok["literal_between_runs"] == [("run", 4, 5), ("lit", 1), ("run", 4, 7)]
    assert tok["run_to_the_end"][-1] == ("run", 4, 6)
    assert tok["stretch_128_then_run"] == [("lit", 128), ("run", 5, K.RUN_VALUE)]
    for s in K.STEP_STARTS:
        assert not sizes(f"run_at_{s}_len_2", "run")
        assert sizes(f"run_at_{s}_len_3", "run") == [3]
        assert sizes(f"run_at_{s}_len_130", "run") == [127, 3]
        assert sum(sizes(f"run_at_{s}_len_3", "lit")[:-1]) == s   # the run starts at byte s


def test_accumulators_of_rows_carry_the_rows():
    for w, (names, stacked) in K.by_width().items():
        for others in ("random", "constant"):
            px = R.rgbe(K.accumulator_of_rows(stacked, others), 1.0)
            assert np.array_equal(px[..., 0], stacked) and (px[..., 3] == 129).all()


def test_crafted_accumulator_reaches_its_cases():
    acc = K.accumulator()
    px = R.rgbe(acc, 1.0).reshape(-1, 4)
    flat = acc.reshape(-1, 3)
    assert set(px[:, 3]) >= set(range(-99 + 128, 127 + 128)) | {0}          # every exponent; 2^127 wraps to 0
    below = flat.max(axis=1).astype(np.float64) < 1e-32
    assert (px[below] == 0).all() and (px[~below, :3].max(axis=1) >= 128).all()
    t = np.float32(1e-32)
    assert float(np.nextafter(t, np.float32(0))) < 1e-32 <= float(t)         # the threshold lies between two floats
    i = int(np.flatnonzero((flat == np.array([1.0, -3.7 / 128, 0.25], np.float32)).all(axis=1))[0])
    assert px[i].tolist() == [128, 0, 32, 129]        # G: -3.7 -> -3 -> 0, the host library's saturating narrowing
    i = int(np.flatnonzero((flat == np.array([1.0, 0.25, -3.7 / 128], np.float32)).all(axis=1))[0])
    assert px[i].tolist() == [128, 32, 253, 129]      # B: -3.7 -> -3 -> 253, the low byte of its scalar conversion
    neg = (flat < 0).any(axis=1) & ~below
    assert neg.sum() >= 6 and (flat[neg] * 256.0 > -2.0 ** 31).all()
    for k in range(3):
        assert (np.argmax(px[~below, :3], axis=1) == k).any()


@pytest.mark.parametrize("samples", K.ACC_SAMPLES)
def test_file_equals_the_host_library_on_the_crafted_accumulator(samples):
    from cuda_pathtracer_amd import encode_hdr
    acc = K.accumulator()
    want = encode_hdr(acc, samples)
    assert R.encode(acc, samples) == want
    assert R.encode(np.ascontiguousarray(acc[:, ::-1]), samples, mirror_x=False) == want
    assert len(want) <= R.bound(acc.shape[1], acc.shape[0])


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (8, 1), (9, 2), (64, 1), (65, 3), (130, 2), (257, 5), (700, 50)])
def test_file_equals_the_host_library_and_the_oracle(w, h):
    from cuda_pathtracer_amd import encode_hdr
    acc = K.noisy(w, h)
    got = R.encode(acc, 3.0)
    assert got == encode_hdr(acc, 3.0)
    assert len(got) <= R.bound(w, h)
    if w * h <= 2000:
        assert got == hdr_oracle.encode_hdr(acc, 3.0)


def test_bound_is_the_formula():
    from cuda_pathtracer_amd import HdrParams
    from cuda_pathtracer_amd import _native as N
    L = N.lib()
    e = C.c_void_p()
    p = HdrParams.default()
    for w, h in [(1, 1), (7, 5), (8, 1), (127, 3), (128, 3), (129, 3), (800, 800), (3840, 2160), (32767, 2), (32768, 2)]:
        head = len(R.header(w, h))
        want = head + (4 * w * h if w < 8 or w >= 32768 else h * (4 + 4 * (w + -(-w // 128))))
        assert R.bound(w, h) == want
        assert L.pt_hdr_enc_create(w, h, C.byref(p), C.byref(e)) == 0
        assert L.pt_hdr_enc_bound(e) == want
        assert L.pt_hdr_enc_destroy(e) == 0


def test_argument_errors_need_no_device():
    from cuda_pathtracer_amd import HdrParams
    from cuda_pathtracer_amd import _native as N
    L = N.lib()
    e = C.c_void_p()
    d = HdrParams.default()
    assert d.mirror_x == 0 and not any(d.reserved)
    assert L.pt_hdr_enc_create(8, 8, None, C.byref(e)) == 1 and L.pt_hdr_enc_create(8, 8, C.byref(d), None) == 1
    for w, h in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert L.pt_hdr_enc_create(w, h, C.byref(d), C.byref(e)) == 1
    p = HdrParams.default()
    p.reserved[3] = 1
    assert L.pt_hdr_enc_create(8, 8, C.byref(p), C.byref(e)) == 1
    # The byte offsets are int32: the bound must stay below 2^31.  Coded rows, 16384 wide: a row takes
    # 4 + 4 * (16384 + 128) = 66052 bytes, so 32512 rows and the header stay 905 bytes below 2^31 and 32513 do not.
    assert R.bound(16384, 32512) == 2 ** 31 - 905 and R.bound(16384, 32513) >= 2 ** 31
    assert L.pt_hdr_enc_create(16384, 32513, C.byref(d), C.byref(e)) == 1
    assert L.pt_hdr_enc_create(16384, 32512, C.byref(d), C.byref(e)) == 0
    assert L.pt_hdr_enc_bound(e) == R.bound(16384, 32512) and L.pt_hdr_enc_destroy(e) == 0
    # flat rows: 4 W H, exactly 2^31 at 32768 x 16384 before the header
    assert R.bound(32768, 16383) < 2 ** 31 <= R.bound(32768, 16384)
    assert L.pt_hdr_enc_create(32768, 16384, C.byref(d), C.byref(e)) == 1
    assert L.pt_hdr_enc_create(32768, 16383, C.byref(d), C.byref(e)) == 0 and L.pt_hdr_enc_destroy(e) == 0
    assert L.pt_hdr_enc_bound(None) == 0 and L.pt_hdr_enc_destroy(None) == 0
    # a created object checks an encode's arguments before it touches a device
    assert L.pt_hdr_enc_create(17, 9, C.byref(d), C.byref(e)) == 0
    one = C.c_float(1.0)
    assert L.pt_hdr_enc_accum(e, None, one, None, 0, None, None) == 1
    assert L.pt_hdr_enc_accum(None, 16, one, 16, 64, 16, None) == 1
    assert L.pt_hdr_enc_accum(e, 16, one, 16, -1, 16, None) == 1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.pt_hdr_enc_accum(e, 16, C.c_float(bad), 16, 64, 16, None) == 1, bad
    assert L.pt_hdr_enc_profile_read(e, (C.c_float * 4)()) == 1
    assert L.pt_hdr_enc_profile(None, 1) == 1
    assert L.pt_hdr_enc_destroy(e) == 0
    n = C.c_int64(0)
    buf = (C.c_uint8 * 64)()
    acc = np.ones((8, 8, 3), np.float32)
    assert L.pt_hdr_encode_host(8, 8, None, one, C.byref(d), buf, 64, C.byref(n)) == 1
    assert L.pt_hdr_encode_host(8, 8, acc.ctypes.data, one, C.byref(d), None, 0, C.byref(n)) == 1
    assert L.pt_hdr_encode_host(8, 8, acc.ctypes.data, one, C.byref(d), buf, -1, C.byref(n)) == 1
    assert L.pt_hdr_encode_host(8, 8, acc.ctypes.data, C.c_float(0.0), C.byref(d), buf, 64, C.byref(n)) == 1
    assert L.pt_hdr_encode_host(0, 8, acc.ctypes.data, one, C.byref(d), buf, 64, C.byref(n)) == 1
    assert L.pt_hdr_encode_host(8, 8, acc.ctypes.data, one, None, buf, 64, C.byref(n)) == 1
    assert L.pt_preview_hdr(None, 1, None, None, 0, None, None) == 1
