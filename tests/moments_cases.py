"""The inputs of tests/test_moments_cpu.py (which asserts that each is well posed) and tests/test_moments_gpu.py (which
runs td_sted_topk on them).  A case is (steds [n_windows, T, 2], valid [n_windows, T] or None, win_ptr list or None, K, nms)."""
import functools

import torch

from moments_ref import moments_ref

NEG = float("-inf")


def _random():  # test_eval_path's "random"
    return torch.randn(4, 257, 2, generator=torch.Generator().manual_seed(6)) * 4


def _tails():  # test_eval_path's "tails"
    steds = torch.randn(3, 257, 2, generator=torch.Generator().manual_seed(4)) * 4
    steds[1, 100:] = NEG
    steds[2, 2:] = NEG
    return steds


def _small():
    return torch.randn(3, 33, 2, generator=torch.Generator().manual_seed(1)) * 4


def _windows():
    steds = torch.randn(6, 8, 2, generator=torch.Generator().manual_seed(10)) * 3
    valid = torch.ones(6, 8, dtype=torch.bool)
    valid[2, 5:] = False
    valid[3, 3:] = False
    valid[5, 6:] = False
    return steds, valid


def _three():
    return torch.tensor([[[2.0, 0.0], [0.0, 1.5], [-1.0, 0.5]]])  # (0, 1) > (0, 2) > (1, 2)


def _ties():  # test_hip_sted_decode_first_index_wins_exact_ties
    steds = torch.full((1, 40, 2), -3.0)
    steds[0, [4, 9], 0] = 5.0
    steds[0, [20, 31], 1] = 5.0
    return steds


def _ties3():
    """Three equal starts: when the pick (4, e) leaves, 9 and 70 tie for end e and sit in different lanes of the kernel's walk."""
    steds = torch.full((1, 100, 2), -3.0)
    steds[0, [4, 9, 70], 0] = 5.0
    steds[0, [80, 90], 1] = 5.0
    return steds


def _threshold():
    steds = torch.full((1, 12, 2), -4.0)
    steds[0, 4, 0], steds[0, 6, 0] = 6.0, 3.0
    steds[0, 7, 1], steds[0, 9, 1] = 6.0, 3.0
    steds[0, 10, 1] = -3.5  # without it (6, 10), (6, 11), (7, 9) and (8, 9) tie for the place of the suppressed (6, 9)
    return steds


def limits_case():
    """P = 3840 as 16 windows of 240.  100 < 3000 are the channels' arg-maxima: the first pick.  3200 and 3700 carry the next
    bumps: (100, 3700) scores higher than (3200, 3700) but has IoU 2901 / 3601 with the first pick."""
    steds = torch.randn(16, 240, 2, generator=torch.Generator().manual_seed(8)) * 0.25
    flat = steds.view(3840, 2)
    flat[100, 0], flat[3000, 1] = 8.0, 8.0
    flat[3200, 0], flat[3700, 1] = 6.0, 6.0
    return steds, None, [0, 16], 2, (1, 2)


def _cases():
    w_steds, w_valid = _windows()
    return {
        "k1_random": (_random(), None, None, 1, (1, 2)),
        "k1_tails": (_tails(), None, None, 1, (1, 2)),
        "plain": (_small(), None, None, 6, (1, 1)),
        "nms": (_small(), None, None, 5, (1, 2)),
        "windows": (w_steds, w_valid, [0, 3, 4, 6], 4, (1, 2)),
        "three_plain": (_three(), None, None, 5, (1, 1)),
        "three_nms0": (_three(), None, None, 5, (0, 1)),
        "single_position": (torch.tensor([[[0.5, -0.5]], [[1.0, 2.0]]]), None, None, 5, (1, 2)),
        "threshold_kept": (_threshold(), None, None, 2, (1, 3)),
        "threshold_dropped": (_threshold(), None, None, 2, (33, 100)),
    }


CASES = _cases()
WELL_POSED = sorted(CASES)  # every case that is compared with float64
TIES = (_ties(), None, None, 4, (1, 1))  # exact ties: decided by the order rule, not by a margin
TIES3 = (_ties3(), None, None, 6, (1, 1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pairs, scores, count, smallest margin) of a case, computed once and shared; do not modify."""
    steds, valid, win_ptr, K, nms = {"ties": TIES, "ties3": TIES3}.get(name) or CASES[name]
    return moments_ref(steds, valid, win_ptr, K, nms)
