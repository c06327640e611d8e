"""Several captions per clip (``clip_index``): the pair bookkeeping against plain Python loops, and the variants the multi-sentence path
refuses.  No GPU: the index vectors are built on the host and only their values are looked at."""
import math
from types import SimpleNamespace

import pytest
import torch

DURATIONS, CLIP_INDEX, STRIDE, HW = [8, 6], [1, 0, 0, 1, 0], 4, 4


def _maps(durations=DURATIONS, clip_index=CLIP_INDEX, stride=STRIDE, hw=HW):
    from tubedetr_amd.functional import PairMaps

    return PairMaps(durations, clip_index, stride, hw, "cpu")


def _check_gather_map(gmap, block_of, n_blocks_in, m):
    """src / CSR lists of a RowGatherMap against loops over every row."""
    want_src = []
    for blk in block_of:
        for j in range(m):
            want_src.append(blk * m + j)
    assert gmap.src.dtype == torch.int32 and gmap.src.tolist() == want_src
    assert (gmap.n_in, gmap.n_out) == (n_blocks_in * m, len(block_of) * m)
    ptr, idx = gmap.seg_ptr.tolist(), gmap.seg_idx.tolist()
    assert len(ptr) == gmap.n_in + 1 and ptr[0] == 0 and ptr[-1] == len(idx) == gmap.n_out
    for r in range(gmap.n_in):
        users = [o for o in range(gmap.n_out) if want_src[o] == r]  # in output (= pair) order
        assert idx[ptr[r] : ptr[r + 1]] == users, r
    # the segment sum is the adjoint of the gather
    g = torch.Generator().manual_seed(0)
    rows, grad = torch.randn(gmap.n_in, 3, generator=g), torch.randn(gmap.n_out, 3, generator=g)
    out = rows[gmap.src.long()]
    back = torch.stack([grad[idx[ptr[r] : ptr[r + 1]]].sum(0) for r in range(gmap.n_in)])
    assert abs(float((out * grad).sum()) - float((rows * back).sum())) < 1e-4


def test_pair_bookkeeping_matches_python_loops():
    from tubedetr_amd.models.transformer import Transformer
    from tubedetr_amd.util.misc import LRUCache

    pm = _maps()
    pair_durations = [DURATIONS[c] for c in CLIP_INDEX]
    assert pm.durations == pair_durations == [6, 8, 8, 6, 8]
    t_clip, t = max(DURATIONS), max(pair_durations)
    n_clips = math.ceil(t_clip / STRIDE)
    assert (pm.P, pm.C, pm.t, pm.t_clip, pm.n_clips) == (5, 2, t, t_clip, n_clips) and not pm.identity
    slow_of, frame_of = [], []
    for c in CLIP_INDEX:
        for j in range(n_clips):
            slow_of.append(c * n_clips + j)
        for j in range(t):
            frame_of.append(c * t_clip + j)
    assert pm.slow_of.tolist() == slow_of and pm.frame_of.tolist() == frame_of
    _check_gather_map(pm.slow, slow_of, len(DURATIONS) * n_clips, HW)
    _check_gather_map(pm.frames, frame_of, len(DURATIONS) * t_clip, HW)
    # what the transformer derives from the per-pair durations: frame owners and the time-query mask
    stub = SimpleNamespace(stride=STRIDE, _idx_cache=LRUCache())
    owner, vid_of_clip, vid_of_frame, query_mask, _ = Transformer._indices(stub, pm.durations, n_clips, "cpu")
    want_mask = [[not (j < d or j == 0) for j in range(t)] for d in pair_durations]
    assert query_mask.tolist() == want_mask
    assert owner.tolist() == [p * n_clips + j // STRIDE for p in range(5) for j in range(t)]
    assert vid_of_clip.tolist() == [p for p in range(5) for _ in range(n_clips)]
    assert vid_of_frame.tolist() == [p for p in range(5) for _ in range(t)]


def test_pair_bookkeeping_other_patterns():
    """A clip that no caption names has empty segments; 0, 1, ..., C - 1 is the identity; shorter pairs than the clips' longest keep t."""
    pm = _maps(durations=[8, 6, 7], clip_index=[2, 2, 0])
    assert pm.durations == [7, 7, 8] and not pm.identity
    ptr = pm.frames.seg_ptr.tolist()
    lo, hi = 1 * 8 * HW, 2 * 8 * HW  # clip 1's frame rows
    assert ptr[lo] == ptr[hi] and ptr[-1] == pm.frames.n_out == 3 * 8 * HW
    _check_gather_map(pm.slow, pm.slow_of.tolist(), 3 * 2, HW)
    _check_gather_map(pm.frames, pm.frame_of.tolist(), 3 * 8, HW)
    assert _maps(clip_index=[0, 1]).identity and not _maps(clip_index=[1, 0]).identity and not _maps(clip_index=[0]).identity
    pm = _maps(durations=[8, 6], clip_index=[1, 1])  # t = 6 < t_clip = 8: frame j of a pair is frame j of its clip
    assert pm.t == 6 and pm.frame_of.tolist() == [8 + j for j in range(6)] * 2
    with pytest.raises(IndexError):
        _maps(clip_index=[0, 2])
    with pytest.raises(AssertionError, match="same number of slow clips"):
        _maps(durations=[8, 4], clip_index=[1])  # (such a batch is refused at the clip level too)


@pytest.fixture(scope="module")
def cpu_model():
    import tubedetr_amd
    from tubedetr_amd.models import build_model

    model, _, _ = build_model(tubedetr_amd.default_args(device="cpu", stride=4))
    return model


def _three_ways(model):
    """Every entry into the multi-sentence path; the refusal comes before the inputs are looked at."""
    from tubedetr_amd.models.tubedetr import VideoFeatures

    vf = VideoFeatures(None, None, None, None, None, [4], 4)
    return (lambda: model.encode_video(None, [4]),
            lambda: model(None, [4], ["a"], clip_index=[0]),
            lambda: model(None, None, ["a"], video_features=vf))


def test_unsupported_variants_raise_and_name_the_flag(cpu_model, monkeypatch):
    from tubedetr_amd.models.tubedetr import TubeDETR

    model = cpu_model
    monkeypatch.setattr(model, "stride", 0)
    for call in _three_ways(model):
        with pytest.raises(NotImplementedError, match="--stride 0"):
            call()
    monkeypatch.setattr(model, "stride", 4)
    for mode in ("gating", "transformer", "pool", "noslow"):
        monkeypatch.setattr(model, "fast_mode", mode)
        for call in _three_ways(model):
            with pytest.raises(NotImplementedError, match="--fast_mode " + mode):
                call()
    monkeypatch.setattr(model, "fast_mode", "")

    class Foreign(torch.nn.Module):  # any backbone object that is not this package's Joiner
        num_channels = 8

        def set_compute_dtype(self, dt):
            pass

    other = TubeDETR(Foreign(), model.transformer, 1, stride=4, fast=True)
    for call in _three_ways(other):
        with pytest.raises(NotImplementedError, match="--backbone"):
            call()
    # the transformer itself refuses too (a caller that drives it directly)
    tr = SimpleNamespace(stride=0, fast=False, fast_mode="", compute_dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="--stride 0"):
        type(model.transformer)._encode(tr, torch.zeros(1, 8, 1, 1), None, None, None, None, [1], None, None, None, [0])
