"""Host side of the yuv420p / nv12 source formats of the device-side augmentation (td_clip_resample_src,
include/tubedetr_hip.h): no GPU needed.

* ``yuv_to_rgb8``: the numpy restatement of the header's integer conversion rule that tests/test_yuv_input_gpu.py
  demands bit equality with; here pinned against the Kr / Kb derivation of its coefficients and against the float64
  formula (bound 0.502 of a level: half a level of rounding + the coefficients' own rounding, as the header states).
* the C ABI: struct mirror, argument validation without a launch.
* ``DecodedClip``'s byte accounting.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (matrix, full_range) -> yo, cy, crv, cbu, cgu, cgv: the header's table
COEF = {
    ("bt601", False): (16, 76309, 104597, 132201, 25675, 53279),
    ("bt601", True): (0, 65536, 91881, 116130, 22553, 46802),
    ("bt709", False): (16, 76309, 117489, 138438, 13975, 34925),
    ("bt709", True): (0, 65536, 103206, 121609, 12276, 30679),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def chroma_hw(sh: int, sw: int):
    return (sh + 1) // 2, (sw + 1) // 2


def convert_triples(Y, U, V, matrix: str, full_range: bool) -> np.ndarray:
    """The integer rule on arrays of samples (any common shape) -> (..., 3) uint8."""
    yo, cy, crv, cbu, cgu, cgv = COEF[(matrix, bool(full_range))]
    c = cy * (np.asarray(Y, dtype=np.int32) - yo) + 32768
    d = np.asarray(U, dtype=np.int32) - 128
    e = np.asarray(V, dtype=np.int32) - 128
    rgb = np.stack([(c + crv * e) >> 16, (c - cgu * d - cgv * e) >> 16, (c + cbu * d) >> 16], axis=-1)  # int32 >>: arithmetic
    return np.clip(rgb, 0, 255).astype(np.uint8)


def yuv_to_rgb8(planes, fmt: str, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """planes: (Y (T, sh, sw), U (T, ch, cw), V (T, ch, cw)) for "yuv420p", (Y, UV (T, ch, cw, 2)) for "nv12", uint8 ->
    (T, sh, sw, 3) uint8 rgb.  Pixel (y, x) uses chroma sample (y >> 1, x >> 1)."""
    if fmt == "yuv420p":
        Y, U, V = planes
    else:
        assert fmt == "nv12"
        Y, UV = planes
        U, V = UV[..., 0], UV[..., 1]
    sh, sw = Y.shape[-2:]
    assert U.shape[-2:] == V.shape[-2:] == chroma_hw(sh, sw)
    yy, xx = np.arange(sh) >> 1, np.arange(sw) >> 1
    return convert_triples(Y, U[..., yy, :][..., :, xx], V[..., yy, :][..., :, xx], matrix, full_range)


def float_rgb(Y, U, V, matrix: str, full_range: bool) -> np.ndarray:
    """The textbook float64 formula, clamped to [0, 255] and not rounded."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    cy, s, yo = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    c, d, e = cy * (np.asarray(Y, dtype=np.float64) - yo), (np.asarray(U, dtype=np.float64) - 128.0) * s, np.asarray(V, dtype=np.float64) - 128.0
    e = e * s
    r = c + 2 * (1 - kr) * e
    g = c - 2 * kb * (1 - kb) / kg * d - 2 * kr * (1 - kr) / kg * e
    b = c + 2 * (1 - kb) * d
    return np.clip(np.stack([r, g, b], axis=-1), 0.0, 255.0)


@pytest.mark.parametrize("key", sorted(COEF))
def test_table_coefficients_are_the_rounded_derivation(key):
    matrix, full = key
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    cy, s = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    want = (0 if full else 16, round(65536 * cy), round(65536 * 2 * (1 - kr) * s), round(65536 * 2 * (1 - kb) * s),
            round(65536 * 2 * kb * (1 - kb) / kg * s), round(65536 * 2 * kr * (1 - kr) / kg * s))
    assert COEF[key] == want


def _max_err(axis_values, matrix, full):
    worst, acc = 0.0, 0
    u, v = np.meshgrid(axis_values, axis_values, indexing="ij")
    yo, cy, crv, cbu, cgu, cgv = COEF[(matrix, full)]
    for y in axis_values:  # one Y level at a time: 256 x 256 triples
        got = convert_triples(np.full_like(u, y), u, v, matrix, full).astype(np.float64)
        worst = max(worst, float(np.abs(got - float_rgb(np.full_like(u, y), u, v, matrix, full)).max()))
    for y in (0, 255):  # the accumulators' extremes are at the corners of the cube
        for d in (-128, 127):
            for e in (-128, 127):
                c = cy * (y - yo) + 32768
                acc = max(acc, abs(c + crv * e), abs(c - cgu * d - cgv * e), abs(c + cbu * d))
    return worst, acc


def test_integer_rule_within_half_a_level_of_float64_bt601_limited_full_sweep():
    worst, acc = _max_err(np.arange(256, dtype=np.int32), "bt601", False)
    print(f"bt601 limited, all 2^24 triples: max |integer - float64| = {worst:.4f} levels, max |accumulator| = {acc}")
    assert worst <= 0.502 and acc < 2 ** 31 // 16


@pytest.mark.parametrize("key", [k for k in sorted(COEF) if k != ("bt601", False)])
def test_integer_rule_within_half_a_level_of_float64_sublattice(key):
    axis = np.unique(np.round(np.linspace(0, 255, 64)).astype(np.int32))
    assert len(axis) == 64 and axis[0] == 0 and axis[-1] == 255
    worst, acc = _max_err(axis, *key)
    print(f"{key}: 64^3 sub-lattice: max |integer - float64| = {worst:.4f} levels, max |accumulator| = {acc}")
    assert worst <= 0.502 and acc < 2 ** 31 // 16


def test_restatement_replicates_chroma_and_handles_both_layouts():
    rng = np.random.default_rng(0)
    sh, sw = 5, 7
    ch, cw = chroma_hw(sh, sw)
    Y = rng.integers(0, 256, (2, sh, sw), dtype=np.uint8)
    U, V = rng.integers(0, 256, (2, ch, cw), dtype=np.uint8), rng.integers(0, 256, (2, ch, cw), dtype=np.uint8)
    a = yuv_to_rgb8((Y, U, V), "yuv420p", "bt709", True)
    b = yuv_to_rgb8((Y, np.stack([U, V], axis=-1)), "nv12", "bt709", True)
    assert a.shape == (2, sh, sw, 3) and np.array_equal(a, b)
    for t, y, x in ((0, 0, 0), (1, 4, 6), (1, 3, 5), (0, 2, 1)):
        assert np.array_equal(a[t, y, x], convert_triples(Y[t, y, x], U[t, y // 2, x // 2], V[t, y // 2, x // 2], "bt709", True))
    # grey: U = V = 128 gives R = G = B, limited-range black and white land on 0 and 255
    grey = convert_triples(np.array([16, 235, 126]), 128, 128, "bt601", False)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all() and grey[0, 0] == 0 and grey[1, 0] == 255


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_resample_src_job_mirror_has_the_header_fields():
    from tubedetr_amd import _hip

    src = open(os.path.join(ROOT, "include", "tubedetr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct td_resample_src_job \{(.*?)\} td_resample_src_job;", " ".join(src.split())).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _hip.ResampleSrcJob._fields_]
    for name, value in (("TD_SRC_RGB24", _hip.TD_SRC_RGB24), ("TD_SRC_I420", _hip.TD_SRC_I420), ("TD_SRC_NV12", _hip.TD_SRC_NV12),
                        ("TD_MATRIX_BT601", _hip.TD_MATRIX_BT601), ("TD_MATRIX_BT709", _hip.TD_MATRIX_BT709)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == value
    assert _hip.lib().td_abi_version() == 11 == _hip.EXPECTED_ABI  # an addition within ABI 11


def test_clip_resample_src_rejects_bad_jobs_without_a_launch():
    from tubedetr_amd import _hip
    from tubedetr_amd.augment import ResampleStage, resample_src_job

    L = _hip.lib()
    nb = L.td_clip_resample_src_table_bytes(1)
    assert nb > 0 and L.td_clip_resample_src_table_bytes(0) == 0 and L.td_clip_resample_src_table_bytes(3) >= L.td_clip_resample_table_bytes(3)
    host = (ctypes.c_char * nb)()
    tab = ctypes.addressof(host)

    def call(job, **override):
        for k, v in override.items():
            setattr(job, k, v)
        arr = (_hip.ResampleSrcJob * 1)(job)
        return L.td_clip_resample_src(arr, 1, tab, tab, nb, None)

    ok = ResampleStage(33, 58, 0, 0, 33, 58)

    def job(fmt="yuv420p", stage=ok, **kw):
        return resample_src_job(4096, 2, 36, 64, False, stage, 16, fmt, **kw)

    def err():
        return L.td_last_error()

    # null planes, one message per plane
    assert call(job(), plane0=None) != 0 and b"plane 0 is null" in err()
    assert call(job(), plane1=None) != 0 and b"plane 1 is null" in err()
    assert call(job(), plane2=None) != 0 and b"plane 2 is null" in err()
    assert call(job("nv12"), plane1=None) != 0 and b"plane 1 is null" in err()
    assert call(job("rgb24"), plane0=None) != 0 and b"plane 0 is null" in err()
    assert call(job(), dst=None) != 0 and b"null destination" in err()
    # pitches below the plane's row bytes (Y 64, chroma 32, NV12 chroma 64, rgb24 192)
    assert call(job(), pitch0=63) != 0 and b"pitch 63 of plane 0" in err()
    assert call(job(), pitch1=31) != 0 and b"pitch 31 of plane 1" in err()
    assert call(job(), pitch2=31) != 0 and b"pitch 31 of plane 2" in err()
    assert call(job("nv12"), pitch1=63) != 0 and b"pitch 63 of plane 1" in err()
    assert call(job("rgb24"), pitch0=191) != 0 and b"pitch 191 of plane 0" in err()
    # unknown format / matrix / range
    assert call(job(), fmt=3) != 0 and b"unknown source format" in err()
    assert call(job(), fmt=-1) != 0 and b"unknown source format" in err()
    assert call(job(), matrix=2) != 0 and b"unknown colour matrix" in err()
    assert call(job(), full_range=2) != 0 and b"unknown colour matrix" in err()
    # frame stride smaller than a plane needs (Y: 36 rows of 64)
    assert call(job(), frame_stride=36 * 64 - 1) != 0 and b"frame stride" in err() and b"plane 0" in err()
    assert call(job(), pitch1=200, frame_stride=36 * 64) != 0 and b"frame stride" in err() and b"plane 1" in err()
    # the checks shared with td_clip_resample
    assert call(job(stage=ResampleStage(33, 58, 30, 0, 4, 58))) != 0 and b"window" in err()
    assert call(job(stage=ResampleStage(33, 58, 0, 50, 33, 9))) != 0 and b"window" in err()
    assert call(job(), T=-1) != 0 and b"negative frame count" in err()
    assert call(job(planar=True, H=33, W=58, mask=None)) != 0 and b"mask" in err()
    assert call(job(planar=True, H=32, W=58, mask=16)) != 0 and b"planar" in err()
    assert call(job(), sw=8193) != 0 and b"sizes" in err()
    assert call(job(), flip=2) != 0 and b"flip" in err()
    assert L.td_clip_resample_src(None, 1, tab, tab, nb, None) != 0
    arr = (_hip.ResampleSrcJob * 1)(job())
    assert L.td_clip_resample_src(arr, 1, tab, tab, nb - 1, None) != 0 and b"table" in err()
    assert err().startswith(b"td_clip_resample_src:")
    # T = 0 is a valid job that launches nothing
    assert call(job(), T=0) == 0


def test_src_job_builder_defaults_are_the_tight_packing():
    from tubedetr_amd import _hip
    from tubedetr_amd.augment import ResampleStage, resample_src_job

    st = ResampleStage(5, 7, 0, 0, 5, 7)
    j = resample_src_job(1000, 2, 37, 51, True, st, 16, "yuv420p", "bt709", True)
    assert (j.fmt, j.matrix, j.full_range, j.flip) == (_hip.TD_SRC_I420, _hip.TD_MATRIX_BT709, 1, 1)
    assert (j.plane0, j.plane1, j.plane2) == (1000, 1000 + 37 * 51, 1000 + 37 * 51 + 19 * 26)
    assert (j.pitch0, j.pitch1, j.pitch2, j.frame_stride) == (51, 26, 26, 37 * 51 + 2 * 19 * 26)
    j = resample_src_job(1000, 2, 37, 51, False, st, 16, "nv12")
    assert (j.fmt, j.plane0, j.plane1, j.plane2) == (_hip.TD_SRC_NV12, 1000, 1000 + 37 * 51, None)
    assert (j.pitch0, j.pitch1, j.frame_stride) == (51, 52, 37 * 51 + 2 * 19 * 26)
    j = resample_src_job(1000, 2, 37, 51, False, st, 16)
    assert (j.fmt, j.plane0, j.pitch0, j.frame_stride) == (_hip.TD_SRC_RGB24, 1000, 153, 153 * 37)
    with pytest.raises(ValueError):
        resample_src_job(1000, 2, 37, 51, False, st, 16, "yuv444p")


# ---- host accounting --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["yuv420p", "nv12"])
@pytest.mark.parametrize("hw", [(36, 64), (37, 51), (1, 1), (2, 3)])
def test_decoded_clip_bytes_per_frame(hw, fmt):
    from tubedetr_amd.augment import DecodedClip

    h, w = hw
    want = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    clip = DecodedClip(np.zeros(3 * want, dtype=np.uint8), 3, h, w, fmt)
    assert clip.nbytes_per_frame == want and clip.nbytes == 3 * want
    with pytest.raises(ValueError):
        DecodedClip(np.zeros(3 * want + 1, dtype=np.uint8), 3, h, w, fmt)


def test_decoded_clip_rgb24_and_bad_arguments():
    from tubedetr_amd.augment import DecodedClip

    clip = DecodedClip(np.zeros((2, 5, 7, 3), dtype=np.uint8), 2, 5, 7, "rgb24")
    assert clip.nbytes_per_frame == 105 and clip.data.shape == (210,)
    with pytest.raises(ValueError):
        DecodedClip(np.zeros(10, dtype=np.uint8), 1, 2, 2, "yuv422p")
    with pytest.raises(ValueError):
        DecodedClip(np.zeros(6, dtype=np.uint8), 1, 2, 2, "yuv420p", matrix="bt2020")
    with pytest.raises(ValueError):
        DecodedClip(np.zeros(6, dtype=np.float32), 1, 2, 2, "yuv420p")
