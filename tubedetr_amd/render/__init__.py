"""Grounded tubes drawn into decoded frames on the device (td_tube_overlay, csrc/overlay.hip: ``annotate``, render/overlay.py; K
labelled tubes and a moment timeline in one pass: td_tube_overlay_multi, csrc/overlay_multi.hip: ``annotate_tubes``,
render/overlay_multi.py), cropped out of them (td_tube_crop, csrc/tube_crop.hip: ``crop_tubes``, render/crop.py) and hidden in
them (td_tube_redact, csrc/redact.hip: ``redact``, render/redact.py); and the stage in front of the three: ``densify``
(td_tube_densify, csrc/tube_dense.hip, render/dense.py) interpolates the tube rows, one per SAMPLED frame, to one box per DECODED
frame, ``frame_stats`` / ``shot_cuts`` (td_frame_stats, td_shot_cuts, csrc/frame_stats.hip, render/shots.py) find the hard cuts
in the frames, at which ``densify(shots=...)`` (td_tube_densify_shots) stops, and ``follow`` (td_tube_follow,
csrc/tube_follow.hip, render/follow.py) moves the in-between boxes onto the object.  The stage behind them all is ``export``
(td_frame_export, csrc/frame_export.hip, render/export.py): the frames of the answer, downscaled, in the pixel format the encoder
wants, padded to even sides - what crosses to the host is the proxy, not the decoded clip.

The reference shows an answer on the host: demo_stvg.py:152-194 and server_stvg.py:218-257 re-decode the video to JPEGs,
open every frame in matplotlib, draw one rectangle and save the JPEG again.  Here the decoded frames stay on the device in
the decoder's own pixel format (``DeviceFrames``, render/frames.py); ``annotate`` writes the boxes ``PostProcess`` returned, the
span ``sted_decode`` returned and - optionally - the decoder's cross-attention (``heat_from_attention``) into them in ONE launch
for any number of clips, and the result goes to an encoder pipe as it is.  The pixel rule is exact integer arithmetic and is
stated in include/tubedetr_hip.h; so is the colour conversion of ``color_in_space``.

Every wrapper reads its arguments through render/clips.py, checks all of them for all clips before it allocates, and launches
once through tubedetr_amd/frame_jobs.py, whose raw launchers are re-exported here.
"""
from ..frame_jobs import (MAX_MAP, MAX_MARGIN_DEN, MAX_RECTS, MAX_SIDE, _JOB_TYPES, _frame_bytes, frame_export, launch_frame_stats, launch_shot_cuts, tube_crop,  # noqa: F401
                          tube_densify, tube_densify_shots, tube_follow, tube_overlay, tube_overlay_multi, tube_redact)
from .crop import MAX_CROP_SIDE, MAX_CROP_SRC_COLS, TubeCrops, crop_job, crop_tubes  # noqa: F401
from .dense import DENSE_MODES, MAX_DENSE_STEP, MAX_DENSE_T, MAX_FRAME_NO, MAX_SMOOTH, DenseTubes, dense_job, densify  # noqa: F401
from .export import MAX_EXPORT_RESIZE_PIXELS, MAX_EXPORT_SRC_COLS, _export_size, export, export_job, moment_take  # noqa: F401
from .follow import MAX_FOLLOW_ACCEPT, MAX_FOLLOW_RADIUS, MAX_FOLLOW_REACH, FollowedTubes, anchors, follow, follow_job  # noqa: F401
from .frames import DeviceFrames, _forward_coefficients, color_in_space  # noqa: F401
from .overlay import TubeStyle, annotate, heat_from_attention, overlay_job  # noqa: F401
from .overlay_multi import (FONT_H, FONT_W, MAX_LABEL_CHARS, MAX_LANE_H, MAX_TAG_H, MAX_TAG_SCALE, MAX_TAG_W, MAX_TIMELINE_ROWS, PALETTE, _FONT, TubeSetStyle,  # noqa: F401
                            annotate_tubes, label_tags, overlay_multi_job)
from .redact import REDACT_MODES, redact, redact_job  # noqa: F401
from .shots import (MAX_CUT_FRACTION, MAX_CUT_T, MAX_CUT_WINDOW, MAX_STAT_PIXELS, MAX_STAT_STEP, STAT_BINS, FrameStats, Shots, cuts_job, frame_stats,  # noqa: F401
                    sampled_pixels, shot_cuts, stats_job)
