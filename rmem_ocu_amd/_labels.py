"""Argument checks and small rules the modules on uint8 label stacks share (pairs, components, tubes, polygons, rle, the label part of
evaluator, distance, surface, skeleton, shapes): integers in a range, connectivity, the stack and its limits, the sides the separable
transforms take, a tensor that goes with a stack, a pair of stacks, the workspace budget of a call that
passes over a stack, the keys of un-squeezed objects, the boundary P / R / F.  Streams, workspaces and packed files are _codec's."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._codec import uint8_stack
from ._lib import RmemError

MAX_FRAMES, MAX_PIXELS = 65535, 1 << 26      # csrc/label_wave.h: kMaxFrames, kMaxPixels
MAX_SIDE = 16384                             # csrc/label_sep.h: kMaxSide, the separable transforms (distance, surface)
WORKSPACE_CAP = 256 << 20                    # bytes one pass over a stack keeps, unless one frame needs more


def is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def int_in(what: str, name: str, v, lo: int, hi: int, must_be: str = 'an integer in') -> int:
    if not is_int(v) or not lo <= int(v) <= hi:
        raise RmemError(f'{what}: {name} must be {must_be} {lo}..{hi} (got {v!r})')
    return int(v)


def connectivity(what: str, v) -> int:
    if not is_int(v) or int(v) not in (4, 8):
        raise RmemError(f'{what}: connectivity must be 4 or 8 (got {v!r})')
    return int(v)


def stack(what: str, t, name: str = 'labels') -> torch.Tensor:
    """_codec.uint8_stack's [n, H, W] view, contiguous, within the limits of the kernels that walk label stacks"""
    a = uint8_stack(t, what, name).contiguous()
    n, H, W = a.shape
    if H * W > MAX_PIXELS or n > MAX_FRAMES:
        raise RmemError(f'{what}: {name} of {n} x {H} x {W} are too large (H * W at most 2^26, at most 65535 frames)')
    return a


def geometry(what: str, a: torch.Tensor) -> Tuple[int, int, int]:
    """(n, H, W) of a stack() view whose sides the separable transforms take"""
    n, H, W = a.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise RmemError(f'{what}: frames of {H} x {W} are too large (H and W at most {MAX_SIDE})')
    return n, H, W


def like_labels(what: str, t, name: str, dtype: torch.dtype, labels: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """t, a tensor the caller passed to go with `labels` (whose stack() view is a), viewed to a's shape; refused unless it is a
    contiguous tensor of that dtype, of the labels' shape, on their device"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != a.device or t.shape != labels.shape or not t.is_contiguous():
        raise RmemError(f'{what}: {name} must be a contiguous {str(dtype)[6:]} tensor of the labels\' shape on their device')
    return t.view(a.shape)


def stack_pair(what: str, a_u8, b_u8, names: Tuple[str, str] = ('a', 'b'), devices: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """two stacks of one shape on one device, contiguous; devices: whether the refusal names them"""
    a, b = uint8_stack(a_u8, what, names[0]), uint8_stack(b_u8, what, names[1])
    if a_u8.shape != b_u8.shape or a.device != b.device:
        got = [f'{tuple(t.shape)} on {t.device}' if devices else f'{tuple(t.shape)}' for t in (a_u8, b_u8)]
        raise RmemError(f'{what}: {names[0]} and {names[1]} must have one shape, [n, H, W] or [H, W], on one device '
                        f'(got {got[0]} and {got[1]})')
    return a.contiguous(), b.contiguous()


def frames_per_pass(what: str, n: int, per_frame: int, workspace_bytes, noun: str) -> Tuple[int, int]:
    """(byte budget, frames per pass) of a call that keeps per_frame bytes per frame of an n-frame stack.  workspace_bytes None:
    what the whole stack needs, WORKSPACE_CAP at most, one frame's bytes at least; anything below one frame's bytes is refused
    (noun: what the message calls those)."""
    if workspace_bytes is None:
        workspace_bytes = max(per_frame, min(n * per_frame, WORKSPACE_CAP))
    elif not is_int(workspace_bytes) or workspace_bytes < per_frame:
        raise RmemError(f'{what}: workspace_bytes must be an integer of at least {noun}, {per_frame} bytes (got {workspace_bytes!r})')
    return int(workspace_bytes), int(min(n, workspace_bytes // per_frame))


def object_keys(num: int, squeeze_idx: Optional[Sequence[int]] = None) -> Dict[int, int]:
    """{id: key} of the objects 1..num in ascending ids: the id itself, or squeeze_idx[id] (save_masks' un-squeeze), ids beyond
    squeeze_idx's length left out"""
    if squeeze_idx is None:
        return {i: i for i in range(1, num + 1)}
    return {i: int(squeeze_idx[i]) for i in range(1, min(num + 1, len(squeeze_idx)))}


def boundary_prf(n_fg, n_gt, fg_m, gt_m) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(P, R, F) of f_measure from float64 arrays of one shape: the boundary pixels of the prediction and of the annotation, and
    how many of each lie within the other's dilated boundary.  P = fg_m / n_fg, R = gt_m / n_gt, F = 2PR / (P + R), and the edge
    cases: no prediction boundary -> (1, 0, 0); no annotation boundary -> (0, 1, 0); neither -> (1, 1, 1); both, without a match
    -> (0, 0, 0).  (n_fg, n_gt, fg_m, gt_m) = (4, 8, 2, 2) -> (0.5, 0.25, 1 / 3)."""
    P = np.where(n_fg > 0, np.where(n_gt > 0, fg_m / np.maximum(n_fg, 1.0), 0.0), 1.0)
    R = np.where(n_gt > 0, np.where(n_fg > 0, gt_m / np.maximum(n_gt, 1.0), 0.0), 1.0)
    return P, R, np.where(P + R == 0, 0.0, 2.0 * P * R / np.where(P + R == 0, 1.0, P + R))
