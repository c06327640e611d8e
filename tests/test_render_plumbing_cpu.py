"""The plane plumbing of every frame-job builder (tubedetr_amd.render's ``*_job`` functions and augment's ``resample_src_job``):
which addresses, pitches and frame stride a job record carries for rgb24, yuv420p and nv12 frames, tightly packed and with
explicit planes.  The expected numbers are literal arithmetic written here, for 6 x 8 frames and for the odd size 5 x 7, whose
chroma planes are still 3 x 4 (the (x + 1) // 2 rounding).  No device: the addresses are made up, as in test_frame_jobs_cpu.py."""
import pytest

SRC, DST, AUX = 1 << 20, 1 << 24, 1 << 26
T = 2

# (pix_fmt, h, w) -> (plane offsets from the base, tight pitches, frame bytes)
TIGHT = {
    ("rgb24", 6, 8): ([0], [24], 144),                       # 6 rows of 3 * 8
    ("yuv420p", 6, 8): ([0, 48, 60], [8, 4, 4], 72),         # Y 6 x 8 = 48, U and V 3 x 4 = 12 each
    ("nv12", 6, 8): ([0, 48], [8, 8], 72),                   # Y 48, UV 3 rows of 2 * 4
    ("rgb24", 5, 7): ([0], [21], 105),                       # 5 rows of 3 * 7
    ("yuv420p", 5, 7): ([0, 35, 47], [7, 4, 4], 59),         # Y 5 x 7 = 35, U and V still 3 x 4: 35 + 24
    ("nv12", 5, 7): ([0, 35], [7, 8], 59),
}
GEOMETRIES = sorted(TIGHT)
WRONG_COUNT = "one address and one pitch per plane, and the frame stride"


def _stage():
    from tubedetr_amd.augment import ResampleStage

    return ResampleStage(4, 4, 0, 0, 4, 4)


def _build(name, fmt, h, w, src=SRC, dst=DST, **planes):
    """One job of builder ``name`` for T frames of h x w; ``planes`` are the builder's own plane keywords."""
    from tubedetr_amd import augment, render

    if name == "overlay":
        return render.overlay_job(src, T, h, w, dst, fmt, boxes=AUX, n_tube=2, **planes)
    if name == "overlay_multi":
        return render.overlay_multi_job(src, T, h, w, dst, fmt, boxes=AUX, n_tube=2, **planes)
    if name == "redact":
        return render.redact_job(src, T, h, w, AUX, 2, 1, dst, fmt, mode="fill", **planes)
    if name == "crop":
        return render.crop_job(src, T, h, w, AUX, 2, dst, (4, 4), fmt, **planes)
    if name == "stats":
        return render.stats_job(src, T, h, w, fmt, hist=AUX, **planes)
    if name == "follow":
        return render.follow_job(src, T, h, w, AUX, AUX + 4096, AUX + 8192, 1, fmt, **planes)
    if name == "export":
        return render.export_job(src, T, h, w, dst, fmt, **planes)
    assert name == "resample_src"
    return augment.resample_src_job(src, T, h, w, False, _stage(), dst, fmt, **planes)


# builder -> the stems of the plane sets it describes ("": plane0 / pitch0 / frame_stride, and planes= / pitches= / frame_stride=)
STEMS = {"overlay": ("src", "dst"), "overlay_multi": ("src", "dst"), "redact": ("src", "dst"), "export": ("src", "dst"), "stats": ("src",), "follow": ("src",),
         "crop": ("",), "resample_src": ("",)}
IN_PLACE = ("overlay", "overlay_multi", "redact")
CASES = [(b, f, h, w) for b in sorted(STEMS) for f, h, w in GEOMETRIES]


def _read(job, stem):
    u = stem + "_" if stem else ""
    planes = [getattr(job, f"{stem}{k}" if stem else f"plane{k}") for k in range(3)]
    return planes, [getattr(job, f"{u}pitch{k}") for k in range(3)], getattr(job, f"{u}frame_stride")


def _kw(stem, planes, pitches, stride):
    u = stem + "_" if stem else ""
    return {u + "planes": planes, u + "pitches": pitches, u + "frame_stride": stride}


def _padded(values, fill):
    return list(values) + [fill] * (3 - len(values))


@pytest.mark.parametrize("builder,fmt,h,w", CASES)
def test_tightly_packed(builder, fmt, h, w):
    offs, pitches, frame = TIGHT[(fmt, h, w)]
    job = _build(builder, fmt, h, w)
    for stem in STEMS[builder]:
        base = DST if stem == "dst" else SRC
        assert _read(job, stem) == (_padded([base + o for o in offs], None), _padded(pitches, 0), frame), stem


@pytest.mark.parametrize("builder,fmt,h,w", CASES)
def test_explicit_planes(builder, fmt, h, w):
    n = len(TIGHT[(fmt, h, w)][0])
    kw, want = {}, {}
    for i, stem in enumerate(STEMS[builder]):
        planes, pitches, stride = [AUX + 65536 * (3 * i + k) for k in range(n)], [64, 32, 48][:n], 9999 + i
        kw.update(_kw(stem, planes, pitches, stride))
        want[stem] = (_padded(planes, None), _padded(pitches, 0), stride)
    job = _build(builder, fmt, h, w, **kw)
    for stem in STEMS[builder]:
        assert _read(job, stem) == want[stem], stem


@pytest.mark.parametrize("builder,fmt,h,w", CASES)
def test_explicit_planes_equal_to_the_tight_ones_give_the_same_bytes(builder, fmt, h, w):
    offs, pitches, frame = TIGHT[(fmt, h, w)]
    kw = {}
    for stem in STEMS[builder]:
        base = DST if stem == "dst" else SRC
        kw.update(_kw(stem, [base + o for o in offs], pitches, frame))
    assert bytes(_build(builder, fmt, h, w, **kw)) == bytes(_build(builder, fmt, h, w))


@pytest.mark.parametrize("fmt,h,w", GEOMETRIES)
def test_explicit_pitches_alone_keep_the_tight_addresses(fmt, h, w):
    offs, pitches, frame = TIGHT[(fmt, h, w)]
    n = len(offs)
    job = _build("stats", fmt, h, w, src_pitches=[64, 32, 48][:n])
    assert _read(job, "src") == (_padded([SRC + o for o in offs], None), _padded([64, 32, 48][:n], 0), frame)


@pytest.mark.parametrize("builder", IN_PLACE)
@pytest.mark.parametrize("fmt,h,w", GEOMETRIES)
def test_in_place_copies_the_src_description(builder, fmt, h, w):
    offs, pitches, frame = TIGHT[(fmt, h, w)]
    job = _build(builder, fmt, h, w, dst=None)
    assert _read(job, "dst") == _read(job, "src") == (_padded([SRC + o for o in offs], None), _padded(pitches, 0), frame)
    n = len(offs)
    planes = [AUX + 4096 * k for k in range(n)]
    job = _build(builder, fmt, h, w, dst=None, **_kw("src", planes, [64, 32, 48][:n], 7777))
    assert _read(job, "dst") == _read(job, "src") == (_padded(planes, None), _padded([64, 32, 48][:n], 0), 7777)
    # a dst of its own beside explicit src planes is described on its own
    job = _build(builder, fmt, h, w, **_kw("src", planes, [64, 32, 48][:n], 7777))
    assert _read(job, "dst") == (_padded([DST + o for o in offs], None), _padded(pitches, 0), frame)


@pytest.mark.parametrize("builder", sorted(STEMS))
def test_wrong_plane_count_is_refused(builder):
    for stem in STEMS[builder]:
        for kw in (_kw(stem, [AUX, AUX + 4096], None, 100),                    # two addresses for the three planes of yuv420p
                   _kw(stem, None, [8, 4], None),                             # two pitches
                   _kw(stem, [AUX, AUX + 4096, AUX + 8192], None, None)):     # planes without the frame stride
            with pytest.raises(ValueError, match=WRONG_COUNT):
                _build(builder, "yuv420p", 6, 8, **kw)
        with pytest.raises(ValueError, match=WRONG_COUNT):
            _build(builder, "rgb24", 6, 8, **_kw(stem, [AUX, AUX + 4096], [24, 24], 144))


def test_export_describes_two_geometries():
    """``export_job``'s two sides differ: 5 x 7 yuv420p frames into 6 x 8 nv12 frames."""
    from tubedetr_amd import render

    job = render.export_job(SRC, T, 5, 7, DST, "yuv420p", "nv12", frame_size=(6, 8))
    assert _read(job, "src") == ([SRC, SRC + 35, SRC + 47], [7, 4, 4], 59)
    assert _read(job, "dst") == ([DST, DST + 48, None], [8, 8, 0], 72)


def test_builders_without_frames_and_the_record_of_every_entry_point():
    from tubedetr_amd import _hip, render

    d = render.dense_job(AUX, 2, T, DST)
    assert (d.boxes, d.dense, d.n_tube, d.T, d.K) == (AUX, DST, 2, T, 1)
    c = render.cuts_job(AUX, AUX + 4096, T, 48, DST, DST + 4096, DST + 8192)
    assert (c.hist, c.sad, c.T, c.N, c.cut, c.shot, c.n_shots) == (AUX, AUX + 4096, T, 48, DST, DST + 4096, DST + 8192)
    kinds = {"td_tube_overlay": "OverlayJob", "td_tube_overlay_multi": "OverlayMultiJob", "td_tube_crop": "CropJob", "td_tube_redact": "RedactJob",
             "td_tube_densify": "DenseJob", "td_frame_stats": "StatsJob", "td_shot_cuts": "CutsJob", "td_tube_follow": "FollowJob", "td_frame_export": "ExportJob"}
    for entry, kind in kinds.items():
        assert render._JOB_TYPES[entry] == kind
        assert _hip._SIGS[entry][0]._type_ is getattr(_hip, kind)
