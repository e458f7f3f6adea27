"""Annotation-driven runs: from a decoded annotation stack to what the slots and the scorer need, on the device.

The reference's dataset class (dataloaders/eval_datasets.py, VOSTest) keeps a running ``curr_objs = [0]`` per sequence and, for
every annotated frame in order, appends the values of ``np.unique(label)`` not yet listed, ascending: the position in that list is
the object's squeezed id, the list itself the ``squeeze_idx`` handed to save_mask.  Here the per-frame ``np.unique`` is a census on
the device (rmem_label_census: area and box per frame and label value, one launch for the whole stack), the rule runs on its
[m, 256] areas on the host (protocol_from_census), and the maps the rule implies -- the squeezed first-frame label and one overlay
per frame on which objects first appear -- come from one more launch (rmem_label_remap with one 256-entry table per frame).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._codec import uint8_stack
from ._lib import RmemError


def label_census(labels_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(area int32 [n, 256], box int32 [n, 256, 4]) of a uint8 device stack [n, H, W] or [H, W]: per frame and label value the
    pixel count and (xmin, ymin, xmax, ymax), (W, H, -1, -1) for a value the frame does not hold (include/rmem.h,
    rmem_label_census).  Both are views of one [n, 256, 5] tensor.  One call on the current stream, no host sync."""
    labels = uint8_stack(labels_u8, 'protocol.label_census').contiguous()
    n, H, W = labels.shape
    out = torch.empty(n, 256, 5, dtype=torch.int32, device=labels.device)
    _lib.check(_lib.lib().rmem_label_census(labels.data_ptr(), n, H, W, out.data_ptr(), torch.cuda.current_stream(labels.device).cuda_stream),
               'rmem_label_census')
    return out[:, :, 0], out[:, :, 1:]


def remap_labels(src_u8: torch.Tensor, luts, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[f] = luts[f][src[f]] (luts [n, 256]) or luts[src[f]] (luts [256]) for a uint8 device stack [n, H, W] or [H, W]
    (rmem_label_remap).  luts: uint8, a numpy array or a tensor on the stack's device.  out: a contiguous uint8 tensor of src's
    shape on its device (src itself: in place); default a new one.  One launch on the current stream, no host sync."""
    src = uint8_stack(src_u8, 'protocol.remap_labels', 'src')
    n, H, W = src.shape
    dev = src.device
    if isinstance(luts, np.ndarray):
        if luts.dtype != np.uint8:
            raise RmemError('protocol.remap_labels: luts must be uint8')
        luts = torch.from_numpy(np.ascontiguousarray(luts)).to(dev)
    if not isinstance(luts, torch.Tensor) or luts.dtype != torch.uint8 or luts.device != dev or tuple(luts.shape) not in ((256,), (n, 256)):
        raise RmemError(f'protocol.remap_labels: luts must be uint8 [256] or [{n}, 256], a numpy array or a tensor on the '
                        'stack\'s device')
    luts = luts.contiguous()
    if out is None:
        src = src.contiguous()
        out = torch.empty_like(src_u8, memory_format=torch.contiguous_format)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or out.shape != src_u8.shape
                or not out.is_contiguous()):
            raise RmemError(f'protocol.remap_labels: out must be a contiguous uint8 {tuple(src_u8.shape)} tensor on the stack\'s device')
        if not src.is_contiguous():
            if out.data_ptr() == src.data_ptr():
                raise RmemError('protocol.remap_labels: in place needs a contiguous stack')
            src = src.contiguous()
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().rmem_label_remap(src.data_ptr(), out.data_ptr(), n, H * W, luts.data_ptr(), int(luts.dim() == 2),
                                           stream.cuda_stream), 'rmem_label_remap')
    for t in (src, luts):
        t.record_stream(stream)
    return out


@dataclass
class ClipProtocol:
    """What a clip's annotations say about its objects.  squeeze_idx: original id of every squeezed id (entry 0 = 0), the list
    save_masks / png.encode_label_stack take; first_frame[k - 1]: the clip frame on which object k (original id squeeze_idx[k])
    first appears; new_frames: the sorted clip frames > 0 on which at least one object first appears.  Tables, uint8 [256], indexed
    by the original id: lut_all -> squeezed id (void -> void, unknown -> 0); lut_first -> squeezed id of the objects of frame 0, 0
    for everything else; lut_new[t] -> squeezed id of the objects with first_frame == t, 0 for everything else."""
    squeeze_idx: List[int]
    num_objs: int
    first_frame: np.ndarray
    new_frames: List[int]
    lut_all: np.ndarray
    lut_first: np.ndarray
    lut_new: Dict[int, np.ndarray]


def _frame_index(frame_index, m: int) -> List[int]:
    idx = list(range(m)) if frame_index is None else [int(i) for i in frame_index]
    if len(idx) != m:
        raise RmemError(f'protocol: frame_index has {len(idx)} entries for {m} annotated frames')
    if m == 0 or idx[0] != 0:
        raise RmemError('protocol: frame_index must start at 0 (the first annotated frame is the clip\'s first frame)')
    if any(b <= a for a, b in zip(idx, idx[1:])):
        raise RmemError('protocol: frame_index must be strictly increasing')
    return idx


def protocol_from_census(area, frame_index: Optional[Sequence[int]] = None, void_label: Optional[int] = 255) -> ClipProtocol:
    """The reference's curr_objs rule on a census: area [m, 256] (host), row j = clip frame frame_index[j] (default range(m);
    strictly increasing from 0, so a clip may pass only the frames that have annotation files).  For each row in order, every
    value v != 0 with area > 0 not yet listed is appended, ascending.  void_label (default 255) is never an object; None treats
    255 as an ordinary id, as the reference does.  A clip without an object on frame 0 raises RmemError."""
    area = np.asarray(area)
    if area.ndim != 2 or area.shape[1] != 256:
        raise RmemError(f'protocol_from_census: area must be [m, 256] (got {area.shape})')
    idx = _frame_index(frame_index, area.shape[0])
    squeeze_idx, first = [0], []
    for j, t in enumerate(idx):
        for v in np.nonzero(area[j] > 0)[0].tolist():            # ascending
            if v != 0 and v != void_label and v not in squeeze_idx:
                squeeze_idx.append(v)
                first.append(t)
    if not first or first[0] != 0:
        raise RmemError('protocol_from_census: no object on frame 0')
    first_frame = np.asarray(first, dtype=np.int64)
    new_frames = sorted({t for t in first if t > 0})
    lut_all = np.zeros(256, dtype=np.uint8)
    lut_first = np.zeros(256, dtype=np.uint8)
    lut_new = {t: np.zeros(256, dtype=np.uint8) for t in new_frames}
    for k in range(1, len(squeeze_idx)):
        v, t = squeeze_idx[k], first[k - 1]
        lut_all[v] = k
        (lut_first if t == 0 else lut_new[t])[v] = k
    if void_label is not None:
        lut_all[void_label] = void_label
    return ClipProtocol(squeeze_idx=squeeze_idx, num_objs=len(squeeze_idx) - 1, first_frame=first_frame, new_frames=new_frames,
                        lut_all=lut_all, lut_first=lut_first, lut_new=lut_new)


def clip_protocol(ann_u8: torch.Tensor, frame_index: Optional[Sequence[int]] = None, void_label: Optional[int] = 255):
    """(ClipProtocol, first_label uint8 [H, W], new_objects {clip frame: uint8 [H, W]}) of a clip's annotation stack ann_u8
    [m, H, W] on the device (evaluator.labels_from_pngs), row j = clip frame frame_index[j].  One census, one [m, 256] readback
    (the only host sync), the rule on the host, one remap launch with a table per row: lut_first on row 0, lut_new[t] on the rows
    of new_frames, zeros elsewhere.  The maps are views of that remapped stack, in squeezed ids.  An overlay holds the objects
    new at its frame and nothing else: a later frame's whole annotation would hand the ground truth to the engine."""
    ann = uint8_stack(ann_u8, 'protocol.clip_protocol', 'annotations').contiguous()
    m = ann.shape[0]
    idx = _frame_index(frame_index, m)
    area = label_census(ann)[0].cpu().numpy()
    proto = protocol_from_census(area, idx, void_label)
    luts = np.zeros((m, 256), dtype=np.uint8)
    luts[0] = proto.lut_first
    row_of = {t: j for j, t in enumerate(idx)}
    for t in proto.new_frames:
        luts[row_of[t]] = proto.lut_new[t]
    maps = remap_labels(ann, luts)
    return proto, maps[0], {t: maps[row_of[t]] for t in proto.new_frames}
