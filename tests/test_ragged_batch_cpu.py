"""Batches of videos with different slow-clip counts: the pure layout function (``functional.batch_layout``), the pair bookkeeping over ragged
clips (``functional.PairMaps``) and the slow-batch frame count check, against values written out by hand.  No GPU, no library."""
import math
from types import SimpleNamespace

import pytest
import torch


def _layout(durations, k):
    from tubedetr_amd.functional import batch_layout

    return batch_layout(durations, k)


def test_layout_of_9_3_6_at_stride_4_by_hand():
    lay = _layout([9, 3, 6], 4)
    assert (lay.b, lay.t, lay.n, lay.F) == (3, 9, 6, 27)
    assert lay.clips == [3, 1, 2] and lay.first_clip == [0, 3, 4]
    assert lay.owner.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2] + [3] * 9 + [4, 4, 4, 4, 5, 5, 5, 5, 5]
    assert lay.vid_of_clip.tolist() == [0, 0, 0, 1, 2, 2]
    assert lay.vid_of_frame.tolist() == [0] * 9 + [1] * 9 + [2] * 9
    F_, T_ = False, True
    assert lay.query_mask.dtype == torch.bool and lay.query_mask.tolist() == [[F_] * 9, [F_, F_, F_, T_, T_, T_, T_, T_, T_], [F_] * 6 + [T_] * 3]
    assert lay.frame_dest.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 20, 21, 22, 23]
    assert lay.clip_of.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5]
    assert lay.table().dtype == torch.int32 and lay.table().tolist() == [[9, 0, 3], [3, 3, 1], [6, 4, 2]]
    # a clip's frames are one contiguous range and every clip owns a frame: what the device builder's closed forms rest on
    owner = lay.owner.tolist()
    assert owner == sorted(owner) and sorted(set(owner)) == list(range(lay.n))


@pytest.mark.parametrize("durations,k", [([8, 6], 4), ([5, 5], 5), ([1], 4)])
def test_equal_clip_counts_keep_the_flat_numbering(durations, k):
    """i * n_clips + j // k, the formula in use before ragged batches (and the reference's)."""
    lay = _layout(durations, k)
    b, t = len(durations), max(durations)
    n_clips = math.ceil(t / k)
    assert lay.clips == [n_clips] * b and lay.n == b * n_clips
    assert lay.owner.tolist() == [i * n_clips + j // k for i in range(b) for j in range(t)]
    assert lay.vid_of_clip.tolist() == [i for i in range(b) for _ in range(n_clips)]
    assert lay.vid_of_frame.tolist() == [i for i in range(b) for _ in range(t)]
    assert lay.query_mask.tolist() == [[not (j < d or j == 0) for j in range(t)] for d in durations]
    assert lay.frame_dest.tolist() == [i * t + j for i, d in enumerate(durations) for j in range(d)]
    assert lay.clip_of.tolist() == [i * n_clips + j // k for i, d in enumerate(durations) for j in range(d)]


def test_transformer_indices_come_from_the_layout():
    from tubedetr_amd.models.transformer import Transformer
    from tubedetr_amd.util.misc import LRUCache

    stub = SimpleNamespace(stride=4, _idx_cache=LRUCache())
    owner, vid_of_clip, vid_of_frame, query_mask, clip_vid_list = Transformer._indices(stub, [9, 3, 6], (3, 1, 2), "cpu")
    lay = _layout([9, 3, 6], 4)
    assert owner.tolist() == lay.owner.tolist() and vid_of_clip.tolist() == clip_vid_list == [0, 0, 0, 1, 2, 2]
    assert vid_of_frame.tolist() == lay.vid_of_frame.tolist() and query_mask.tolist() == lay.query_mask.tolist()


def test_host_replica_maps_follow_a_ragged_owner():
    """The host builder on the ragged owner: gather sources and CSR lists against loops over every row."""
    from tubedetr_amd.functional import ReplicaMaps

    lay = _layout([9, 3, 6], 4)
    hw, L = 2, 3
    S = hw + L
    m = ReplicaMaps(lay.owner, lay.n, hw, L, "cpu")
    owner = lay.owner.tolist()
    assert m.all_src.tolist() == [owner[f] * S + s for f in range(lay.F) for s in range(S)]
    idx, ptr = m.seg_all[0].tolist(), m.seg_all[1].tolist()
    assert len(ptr) == lay.n * S + 1 and ptr[-1] == len(idx) == lay.F * S
    for c in range(lay.n):
        for s in range(S):
            assert idx[ptr[c * S + s] : ptr[c * S + s + 1]] == [f * S + s for f in range(lay.F) if owner[f] == c]


def test_pair_maps_over_ragged_clips_by_hand():
    from tubedetr_amd.functional import PairMaps

    pm = PairMaps([9, 3], [1, 0, 0, 1], 4, 4, "cpu")
    assert pm.durations == [3, 9, 9, 3] and (pm.P, pm.C, pm.t, pm.t_clip) == (4, 2, 9, 9) and not pm.identity
    assert (pm.n_slow, pm.n_pair_slow) == (4, 8)
    assert pm.slow_of.tolist() == [3, 0, 1, 2, 0, 1, 2, 3]
    assert pm.frame_of.tolist() == list(range(9, 18)) + list(range(9)) + list(range(9)) + list(range(9, 18))
    assert pm.slow.src.tolist() == [c * 4 + j for c in [3, 0, 1, 2, 0, 1, 2, 3] for j in range(4)]
    assert (pm.slow.n_in, pm.slow.n_out, pm.frames.n_in, pm.frames.n_out) == (4 * 4, 8 * 4, 18 * 4, 36 * 4)
    # the pair batch is ragged itself: clip counts 1, 3, 3, 1
    lay = _layout(pm.durations, 4)
    assert lay.clips == [1, 3, 3, 1] and lay.n == pm.n_pair_slow
    assert PairMaps([9, 3], [0, 1], 4, 4, "cpu").identity


def test_wrong_slow_frame_count_names_the_expected_count():
    import tubedetr_amd
    from tubedetr_amd.functional import check_slow_count
    from tubedetr_amd.models import build_model

    lay = _layout([9, 3, 6], 4)
    check_slow_count(6, lay)
    with pytest.raises(ValueError, match=r"has 9 frames.* need 6 "):
        check_slow_count(9, lay)
    model, _, _ = build_model(tubedetr_amd.default_args(device="cpu", stride=4))
    d = model.transformer.d_model
    with pytest.raises(ValueError, match=r"has 9 frames.* need 6 "):  # the padded count 3 * ceil(9 / 4): refused before any launch
        model.transformer(torch.zeros(9, d, 1, 1), torch.zeros(9, 1, 1, dtype=torch.bool), model.query_embed.weight, None, ["a", "b", "c"],
                          encode_and_save=True, durations=[9, 3, 6])


def test_ablation_variants_refuse_ragged_clip_counts():
    import tubedetr_amd
    from tubedetr_amd.models import build_model

    model, _, _ = build_model(tubedetr_amd.default_args(device="cpu", stride=4, fast=True, fast_mode="gating"))
    d = model.transformer.d_model
    with pytest.raises(NotImplementedError, match="--fast_mode gating"):
        model.transformer(torch.zeros(6, d, 1, 1), torch.zeros(6, 1, 1, dtype=torch.bool), model.query_embed.weight, None, ["a", "b", "c"],
                          encode_and_save=True, durations=[9, 3, 6])


def test_host_maps_switch():
    from tubedetr_amd import functional as Fk

    before = Fk.host_maps()
    try:
        Fk.set_host_maps(True)
        assert Fk.host_maps()
        Fk.set_host_maps(False)
        assert not Fk.host_maps()
    finally:
        Fk.set_host_maps(before)
