"""Per-sequence evaluation protocol on top of the engines (the caller of the hot path).

Mirrors what networks/managers/evaluator.py:330-568 does for one sequence, without its dataset plumbing:
  * per-sequence gap = max(round(n / 30), 5) (330-335), assigned to every engine (356);
  * one engine per test-time augmentation (342-355): horizontal flip and/or extra scales; every augmentation's
    logits are resized to the original size, flipped back, soft-maxed and averaged, then arg-maxed (427-441)
    -- rmem_tta_merge;
  * a ground-truth label that arrives on a later frame (a new object) is merged over the prediction and the frame is
    re-added as a reference frame to every engine (484-508); otherwise the prediction updates the memory (509-523);
  * masks can be written as palette PNGs (utils/image.py:90-106) and scored with the region similarity J
    (evaluation/source/metrics.py:6-37) -- rmem_mask_iou_counts;
  * whole stacks of predicted masks are written as palette PNGs from the device: the DEFLATE payload of every frame is encoded
    there and only the few KB of each file cross to the host -- rmem_png_encode_labels, save_masks, png.encode_label_stack
    (save_mask, one host mask through Pillow, stays as it is);
  * frames with the predicted masks laid over them (palette tint, black contour: the reference's demo overlay) are written as
    baseline JPEGs from the device, overlay and compression fused in one call -- rmem_jpeg_encode_rgb8, save_overlays,
    jpeg.encode_rgb_stack, jpeg.overlay;
  * annotation files are decoded on the device too: only the compressed bytes cross to it -- rmem_png_decode_labels,
    labels_from_pngs, png.decode_label_stack;
  * whole clips are scored on the device with J and the boundary accuracy F (the benchmark toolkit's db_eval_iou /
    db_eval_boundary and its per-sequence mean, recall and decay) -- rmem_clip_score_counts, score_clip;
  * what the dataset class derives from a sequence's annotations (dataloaders/eval_datasets.py, VOSTest: the object list, the
    squeeze of sparse ids, the first label, objects that appear mid-clip) comes from a census of the decoded stack on the device
    -- rmem_label_census / rmem_label_remap, protocol.py, run_annotated_clips, score_annotated_clip, object_boxes;
  * the other format of the field, COCO run-length masks (BURST / TAO-VOS, YouTube-VIS, SA-V, pycocotools), is written and read
    on the device as well: one string per frame and object out, label stacks in -- rmem_rle_encode_labels /
    rmem_rle_decode_labels, rle.py, rle_results, labels_from_rles;
  * the overlap of EVERY predicted with every annotated object, where the scorer compares id i with id i only, comes from one
    joint histogram per frame built on the device: matching predictions whose ids are not the annotation's, and telling an
    identity swap from a lost object -- rmem_label_pair_census, pairs.py, relabel_to_match, identity_report;
  * the boundary counts of every such pair come from the device as well, and with them the DAVIS unsupervised protocol (proposals
    matched to annotated objects on the mean of J and F) and clip scoring for up to 255 objects -- rmem_pair_boundary_counts,
    pairs.pair_jf, score_unsupervised_clip, score_clip_objects;
  * the distance of every pixel to the nearest pixel of another kind is an exact integer transform on the device, and with it
    the Hausdorff distance of every object and the next click of an interactive protocol -- rmem_label_edt,
    rmem_label_edt_peaks, distance.py, surface_distance, next_clicks;
  * the robust surface distances (95th-percentile Hausdorff, average symmetric surface distance, surface Dice at a tolerance) come
    from a census of surface-to-surface distances on the device -- rmem_label_surface, rmem_label_edt_at, rmem_surface_census,
    surface.py, surface_metrics;
  * the centre line of every object is a thinning on the device (Guo and Hall's rule, bit-identical to a host restatement), and
    with it the scribble of an interactive protocol: the longest path through the skeleton of the largest error --
    rmem_label_thin, rmem_label_pixels_count / _write, skeleton.py, next_scribbles;
  * which pixel the nearest site is, not only how far, comes from the same two passes with the site carried along (ties to the
    first site in raster order), and with the label read there objects grow without overlap, void pixels take the nearest real
    value and sparse seeds become a full label map -- rmem_label_nearest, distance.nearest / grow, expand_masks, fill_void,
    labels_from_seeds;
  * the same with the frame in view: the nearest site by the cheapest path through the pixel grid, whose steps cost by how much
    the picture changes (integers, bit-identical to a host Dijkstra), so seeds grow up to an object's edge, a void rim is split
    along it and the boundaries of delivered labels snap to it -- rmem_label_geodesic_begin / _rounds / _finish,
    distance.geodesic_nearest / geodesic_grow, labels_from_seeds_geodesic, fill_void_geodesic, snap_masks;
  * what shape an object has -- centroid, orientation, axis lengths, solidity, convex hull, VOT's rotated box -- comes from one pass
    over the labels by image rows (exact 64-bit moments, the x extent of every object on every row) and a hull built from those
    extents alone -- rmem_label_moments, rmem_label_hull_count / _offsets / _write, shapes.py, object_shapes, object_centroids,
    rotated_boxes.
"""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _labels, _lib, ops
from ._codec import davis_palette as _davis_palette, workspace
from .clip_runner import clip_gap
from .networks.engines import build_engine


def save_mask(mask_u8: np.ndarray, path: str, squeeze_idx: Optional[Sequence[int]] = None):
    """utils/image.py:90-101: optional un-squeeze of object ids, then an indexed PNG with the DAVIS palette."""
    from PIL import Image
    mask = np.asarray(mask_u8, dtype=np.uint8)
    if squeeze_idx is not None:
        out = np.zeros_like(mask)
        for idx in range(1, len(squeeze_idx)):
            out += ((mask == idx) * squeeze_idx[idx]).astype(np.uint8)
        mask = out
    im = Image.fromarray(mask).convert('P')
    im.putpalette(_davis_palette())
    im.save(path)


def save_masks(labels_u8: torch.Tensor, paths: Sequence[str], squeeze_idx: Optional[Sequence[int]] = None):
    """save_mask for a whole stack of device label maps ([n, H, W] or [H, W] uint8): one indexed PNG with the DAVIS palette per
    path, the un-squeeze of object ids and the compression done on the device (png.encode_label_stack)."""
    from . import png
    files = png.encode_label_stack(labels_u8, squeeze_idx)
    if len(files) != len(paths):
        raise _lib.RmemError(f'save_masks: {len(files)} frames but {len(paths)} paths')
    for path, data in zip(paths, files):
        with open(path, 'wb') as f:
            f.write(data)


def save_overlays(rgb_u8: torch.Tensor, labels_u8: torch.Tensor, paths: Sequence[str], quality: int = 90, alpha: float = 0.4):
    """One baseline .jpg per path of the device frames ([n, H, W, 3] or [H, W, 3] uint8) with the label maps ([n, H, W] or [H, W]
    uint8) laid over them: every object tinted in its DAVIS palette colour, a black contour round it (jpeg.overlay).  Overlay and
    compression run on the device (jpeg.encode_rgb_stack); only the files cross to the host."""
    from . import jpeg
    if labels_u8 is None:
        raise _lib.RmemError('save_overlays: labels must be a uint8 device tensor')
    n = rgb_u8.shape[0] if isinstance(rgb_u8, torch.Tensor) and rgb_u8.dim() == 4 else 1
    if n != len(paths):
        raise _lib.RmemError(f'save_overlays: {n} frames but {len(paths)} paths')
    files = jpeg.encode_rgb_stack(rgb_u8, labels_u8, quality=quality, alpha=alpha)
    for path, data in zip(paths, files):
        with open(path, 'wb') as f:
            f.write(data)


def tta_merge(logits: Sequence[torch.Tensor], flips: Sequence[bool], want_prob: bool = False):
    """logits: per-augmentation [1, nc, H, W] fp32 device tensors -> (label uint8 [H, W], label fp32 [1,1,H,W], prob or None)."""
    n = len(logits)
    nc, H, W = logits[0].shape[1:]
    dev = logits[0].device
    label = torch.empty(H, W, dtype=torch.uint8, device=dev)
    label_f = torch.empty(1, 1, H, W, dtype=torch.float32, device=dev)
    prob = torch.empty(1, nc, H, W, dtype=torch.float32, device=dev) if want_prob else None
    ptrs = (C.c_void_p * n)(*[t.contiguous().data_ptr() for t in logits])
    fl = (C.c_int * n)(*[int(f) for f in flips])
    _lib.check(_lib.lib().rmem_tta_merge(ptrs, fl, n, nc, H, W, label.data_ptr(), label_f.data_ptr(),
                                         None if prob is None else prob.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               'rmem_tta_merge')
    return label, label_f, prob


def region_similarity(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_ids: int = 11, void_label: int = 255) -> Dict[int, float]:
    """J per object id for one mask pair (device uint8 tensors of equal shape); ids absent from both masks are skipped."""
    assert pred_u8.dtype == torch.uint8 and gt_u8.dtype == torch.uint8 and pred_u8.shape == gt_u8.shape
    counts = torch.zeros(2 * num_ids, dtype=torch.int64, device=pred_u8.device)
    _lib.check(_lib.lib().rmem_mask_iou_counts(pred_u8.contiguous().data_ptr(), gt_u8.contiguous().data_ptr(), pred_u8.numel(),
                                               num_ids, void_label, counts.data_ptr(),
                                               torch.cuda.current_stream(pred_u8.device).cuda_stream), 'rmem_mask_iou_counts')
    c = counts.cpu().view(num_ids, 2)
    return {i: (1.0 if c[i, 1] == 0 else float(c[i, 0]) / float(c[i, 1])) for i in range(1, num_ids) if c[i, 1] > 0}


def _label_stacks(pred_u8, gt_u8, what):
    return _labels.stack_pair(what, pred_u8, gt_u8, ('pred', 'gt'), devices=False)


def boundary_radius(H: int, W: int, bound_th: float = 0.008) -> int:
    """f_measure's dilation radius: bound_th when it is >= 1 (an integer then), else ceil(bound_th * image diagonal)."""
    r = _lib.lib().rmem_boundary_radius(int(H), int(W), float(bound_th))
    if r < 0:
        raise _lib.RmemError(f'boundary_radius: bad argument (H={H}, W={W}, bound_th={bound_th})')
    return r


def clip_counts(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_ids: int = 11, void_label: int = 255,
                bound_th: float = 0.008) -> torch.Tensor:
    """The six counts behind F and J per (frame, id): int64 device tensor [n, num_ids, 6] = n_fg, n_gt, fg_match, gt_match,
    J intersection, J union (include/rmem.h, rmem_clip_score_counts).  pred / gt: uint8 device label maps [n, H, W] or [H, W].
    Enqueued on the current stream, no host sync.  The bit-plane workspace is one buffer per (device, stream) that only grows
    (to the longest stack seen), so calls on different streams never share planes."""
    pred, gt = _label_stacks(pred_u8, gt_u8, 'clip_counts')
    n, H, W = pred.shape
    L = _lib.lib()
    radius = boundary_radius(H, W, bound_th)
    nbytes = L.rmem_clip_score_workspace_bytes(n, H, W, int(num_ids))
    if nbytes == 0:
        raise _lib.RmemError(f'clip_counts: num_ids must be in 2..32 (got {num_ids})')
    stream = torch.cuda.current_stream(pred.device)
    ws = workspace('score', pred.device, stream, nbytes)        # the boundary bit planes
    counts = torch.empty(n, int(num_ids), 6, dtype=torch.int64, device=pred.device)
    _lib.check(L.rmem_clip_score_counts(pred.data_ptr(), gt.data_ptr(), n, H, W, int(num_ids), int(void_label), radius,
                                        ws.data_ptr(), counts.data_ptr(), stream.cuda_stream),
               'rmem_clip_score_counts')
    return counts


def scores_from_counts(counts) -> Tuple[np.ndarray, np.ndarray]:
    """counts [n, num_ids, 6] (host) -> (J, F) float64 [n, num_ids].  J = intersection / union, 1 for an empty union
    (db_eval_iou); F = 2PR / (P + R) with f_measure's edge cases: no prediction boundary -> P = 1, R = 0; no annotation boundary
    -> P = 0, R = 1; neither -> P = R = 1; F = 0 when P + R = 0."""
    c = np.asarray(counts).astype(np.float64)
    n_fg, n_gt, fg_m, gt_m, inter, union = (c[..., i] for i in range(6))
    J = np.where(union == 0, 1.0, inter / np.maximum(union, 1.0))
    return J, _labels.boundary_prf(n_fg, n_gt, fg_m, gt_m)[2]


def boundary_accuracy(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_ids: int = 11, void_label: int = 255,
                      bound_th: float = 0.008) -> Dict[int, float]:
    """F per object id for one mask pair (device uint8 tensors of equal shape); ids absent from both masks are skipped."""
    if isinstance(pred_u8, torch.Tensor) and pred_u8.dim() != 2:
        raise _lib.RmemError('boundary_accuracy: one [H, W] mask pair (use clip_counts / score_clip for a stack)')
    c = clip_counts(pred_u8, gt_u8, num_ids, void_label, bound_th).cpu().numpy()
    F = scores_from_counts(c)[1]
    return {i: float(F[0, i]) for i in range(1, num_ids) if c[0, i, 5] > 0}


def sequence_statistics(values: np.ndarray) -> Tuple[float, float, float]:
    """The benchmark's per-sequence summary of one object's per-frame values (db_statistics): mean, recall (share > 0.5) and
    decay (mean of the first of four bins minus mean of the last; bin edges round(linspace(1, len, 5) + 1e-10) - 1, each bin
    inclusive of its end index)."""
    v = np.asarray(values, dtype=np.float64)
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return float(v.mean()), float((v > 0.5).mean()), float(bins[0].mean() - bins[3].mean())


@dataclass
class ClipScore:
    """score_clip's result.  J / F: per-frame values [n, num_objs] of every frame of the stack, column i = object id i + 1;
    frames: the indices the statistics run over; *_obj_*: per object over those frames; J_mean, F_mean, JF_mean, J_recall, ...:
    averaged over objects; J_tail: mean J over the last `tail` share of those frames (VOST's tail measure), averaged over objects."""
    J: np.ndarray
    F: np.ndarray
    frames: np.ndarray
    J_obj_mean: np.ndarray
    J_obj_recall: np.ndarray
    J_obj_decay: np.ndarray
    F_obj_mean: np.ndarray
    F_obj_recall: np.ndarray
    F_obj_decay: np.ndarray
    J_obj_tail: np.ndarray
    J_mean: float
    J_recall: float
    J_decay: float
    F_mean: float
    F_recall: float
    F_decay: float
    JF_mean: float
    J_tail: float
    obj_frames: Optional[List[np.ndarray]] = None   # summarize_scores_per_object: the frames each object's statistics run over


def summarize_scores(J: np.ndarray, F: np.ndarray, frames=slice(1, -1), tail: float = 0.25) -> ClipScore:
    """Host half of score_clip: per-frame J / F [n, num_objs] -> ClipScore.  The tail covers frames int(len * (1 - tail)) .. end
    of the selected frames."""
    J, F = np.asarray(J, dtype=np.float64), np.asarray(F, dtype=np.float64)
    sel = np.arange(J.shape[0])[frames]
    if sel.size == 0 or J.shape[1] == 0:
        raise _lib.RmemError(f'score_clip: no frame or no object to score ({J.shape[0]} frames, {J.shape[1]} objects)')
    if not 0.0 < tail <= 1.0:
        raise _lib.RmemError(f'score_clip: tail must be in (0, 1] (got {tail})')
    js = np.array([sequence_statistics(J[sel, o]) for o in range(J.shape[1])])
    fs = np.array([sequence_statistics(F[sel, o]) for o in range(F.shape[1])])
    jt = J[sel[int(sel.size * (1.0 - tail)):]].mean(axis=0)
    return ClipScore(J=J, F=F, frames=sel, J_obj_mean=js[:, 0], J_obj_recall=js[:, 1], J_obj_decay=js[:, 2], F_obj_mean=fs[:, 0],
                     F_obj_recall=fs[:, 1], F_obj_decay=fs[:, 2], J_obj_tail=jt, J_mean=float(js[:, 0].mean()),
                     J_recall=float(js[:, 1].mean()), J_decay=float(js[:, 2].mean()), F_mean=float(fs[:, 0].mean()),
                     F_recall=float(fs[:, 1].mean()), F_decay=float(fs[:, 2].mean()),
                     JF_mean=float(0.5 * (js[:, 0].mean() + fs[:, 0].mean())), J_tail=float(jt.mean()))


def score_clip(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: Optional[int] = None, frames=slice(1, -1), tail: float = 0.25,
               void_label: int = 255, bound_th: float = 0.008) -> ClipScore:
    """J, F and their per-clip summary for a stack of predicted label maps against the annotation ([n, H, W] uint8, device):
    one clip_counts call and one device-to-host copy.  Objects 1..num_objs are scored on every frame (empty against empty
    scores 1, as the benchmark does); num_objs defaults to the largest non-void id of the annotation (one more scalar read).
    frames: the frames the statistics run over; the default drops the first and the last one, as the semi-supervised protocol does."""
    pred, gt = _label_stacks(pred_u8, gt_u8, 'score_clip')
    if num_objs is None:
        num_objs = int(torch.where(gt == void_label, torch.zeros_like(gt), gt).max().item())
    if not 1 <= num_objs <= 31:
        raise _lib.RmemError(f'score_clip: num_objs must be in 1..31 (got {num_objs})')
    J, F = scores_from_counts(clip_counts(pred, gt, num_objs + 1, void_label, bound_th).cpu().numpy())
    return summarize_scores(J[:, 1:], F[:, 1:], frames, tail)


def _max_object(gt: torch.Tensor, void_label) -> int:
    return int((gt if void_label is None else torch.where(gt == void_label, torch.zeros_like(gt), gt)).max().item())


def _pair_tables(pred, gt, num_a, num_b, void_label, bound_th):
    """pairs.pair_census and pairs.pair_boundary_counts of one pair of stacks, read back: (census, match, bnd_a, bnd_b)"""
    from . import pairs
    census = pairs.pair_census(pred, gt, num_a, num_b)
    tables = pairs.pair_boundary_counts(pred, gt, num_a, num_b, void_label, bound_th)
    return (census.cpu().numpy(),) + tuple(t.cpu().numpy() for t in tables)


def score_clip_objects(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: Optional[int] = None, frames=slice(1, -1),
                       tail: float = 0.25, void_label: Optional[int] = 255, bound_th: float = 0.008) -> ClipScore:
    """score_clip for 1..255 objects: the diagonal of the pair tables (pairs.pair_census, pairs.pair_boundary_counts) pushed
    through scores_from_counts and summarize_scores.  Up to 31 objects every field equals score_clip's bit for bit -- the same
    integers, the same float code -- as long as the annotation holds nothing but 0..num_objs and void_label: an annotated value
    above num_objs that is not void counts nowhere here (pairs.pair_iou's drop_other_b) and as "not the object" there.
    void_label must lie above num_objs; None means no void and is the only choice for 255 objects.  num_objs defaults to the
    largest non-void id of the annotation (one more scalar read)."""
    from . import pairs
    pred, gt = _label_stacks(pred_u8, gt_u8, 'score_clip_objects')
    if num_objs is None:
        num_objs = _max_object(gt, void_label)
    K = _labels.int_in('score_clip_objects', 'num_objs', num_objs, 1, 255, must_be='in')
    census, match, bnd_a, bnd_b = _pair_tables(pred, gt, K, K, void_label, bound_th)
    _, inter, union = pairs.pair_iou(census, drop_other_b=void_label is not None)
    d = np.arange(K)
    counts = np.zeros((pred.shape[0], K + 1, 6), dtype=np.int64)
    counts[:, 1:, 0], counts[:, 1:, 1] = bnd_a[:, 1:], bnd_b[:, 1:]
    counts[:, 1:, 2], counts[:, 1:, 3] = match[:, d + 1, d + 1, 0], match[:, d + 1, d + 1, 1]
    counts[:, 1:, 4], counts[:, 1:, 5] = inter[:, d, d], union[:, d, d]
    J, F = scores_from_counts(counts)
    return summarize_scores(J[:, 1:], F[:, 1:], frames, tail)


def summarize_unsupervised(J: np.ndarray, F: np.ndarray, gt_area: np.ndarray, gt_bnd: np.ndarray, frames=slice(None),
                           tail: float = 0.25) -> Tuple[ClipScore, Dict[int, Optional[int]]]:
    """Host half of score_unsupervised_clip.  J, F: float64 [n, num_pred, num_gt], every proposal against every annotated object
    on every frame (pairs.pair_jf); gt_area, gt_bnd [n, num_gt]: the pixels and the boundary pixels of every annotated object.
    M[i, j] = (mean J + mean F) / 2 over `frames`; pairs.assign picks the one-to-one assignment with the largest total M (every
    proposal or every object gets a partner, whichever are fewer; among equal totals the lexicographically smallest); annotated
    object j is scored by its partner's series, and without one against an empty prediction: J = 1 on the frames where its mask
    is empty, else 0, F = 1 where it has no boundary, else 0 (f_measure with no predicted boundary: P = 1, R = 0) -- the
    toolkit's zero padding.  -> (ClipScore with one column per annotated object, {annotated id: proposal id or None})."""
    from . import pairs
    J, F = np.asarray(J, dtype=np.float64), np.asarray(F, dtype=np.float64)
    area, bnd = np.asarray(gt_area), np.asarray(gt_bnd)
    if J.ndim != 3 or J.shape != F.shape or 0 in J.shape or area.shape != (J.shape[0], J.shape[2]) or bnd.shape != area.shape:
        raise _lib.RmemError(f'score_unsupervised_clip: J and F must be [n, num_pred, num_gt], gt_area and gt_bnd [n, num_gt] '
                             f'(got {J.shape}, {F.shape}, {area.shape}, {bnd.shape})')
    sel = np.arange(J.shape[0])[frames]
    if sel.size == 0:
        raise _lib.RmemError(f'score_unsupervised_clip: no frame to score ({J.shape[0]} frames)')
    M = 0.5 * (J[sel].mean(axis=0) + F[sel].mean(axis=0))
    partner = {j: i for i, j in pairs.assign(M, minimum=-1.0)}        # M >= 0: no chosen pair is left out
    Jo, Fo = np.where(area == 0, 1.0, 0.0), np.where(bnd == 0, 1.0, 0.0)
    for j, i in partner.items():
        Jo[:, j], Fo[:, j] = J[:, i, j], F[:, i, j]
    mapping = {j + 1: (partner[j] + 1 if j in partner else None) for j in range(J.shape[2])}
    return summarize_scores(Jo, Fo, frames, tail), mapping


def score_unsupervised_clip(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_pred: int, num_gt: Optional[int] = None,
                            frames=slice(None), tail: float = 0.25, void_label: Optional[int] = 255, bound_th: float = 0.008,
                            max_proposals: int = 20) -> Tuple[ClipScore, Dict[int, Optional[int]]]:
    """The DAVIS unsupervised protocol for one clip: pred_u8 holds proposals 1..num_pred whose ids mean nothing, gt_u8 annotated
    objects 1..num_gt ([n, H, W] uint8 device stacks; num_gt defaults to the annotation's largest non-void id).  J and F of every
    (proposal, object) pair on every frame (pairs.pair_census, pairs.pair_boundary_counts, pairs.jf_from_tables: two device calls,
    then the readback of the four tables), then summarize_unsupervised: proposals are matched to objects on the mean of J and F, every
    object is scored by its partner, an object without one against an empty prediction.  More than max_proposals proposals raise
    RmemError (the benchmark allows 20).  -> (ClipScore, {annotated id: proposal id or None}); every frame is scored by default,
    as the unsupervised protocol does."""
    from . import pairs
    what = 'score_unsupervised_clip'
    if isinstance(num_pred, (int, np.integer)) and num_pred > max_proposals:
        raise _lib.RmemError(f'{what}: {num_pred} proposals, the protocol allows max_proposals = {max_proposals}')
    pred, gt = _label_stacks(pred_u8, gt_u8, what)
    if num_gt is None:
        num_gt = _max_object(gt, void_label)
    census, match, bnd_a, bnd_b = _pair_tables(pred, gt, num_pred, num_gt, void_label, bound_th)
    J, F = pairs.jf_from_tables(census, match, bnd_a, bnd_b, drop_other_b=void_label is not None)
    gt_area = census.sum(axis=1)[:, 1:int(num_gt) + 1]               # void pixels sit in the "other" column, not here
    return summarize_unsupervised(J, F, gt_area, bnd_b[:, 1:], frames, tail)


def summarize_scores_per_object(J: np.ndarray, F: np.ndarray, first_frames: Sequence[int], tail: float = 0.25) -> ClipScore:
    """Host half of score_annotated_clip: summarize_scores with a frame range per object.  Object k (column k - 1) is scored over
    frames first_frames[k - 1] + 1 .. n - 2: from the frame after the one that shows it to the engine to the last but one, as the
    semi-supervised protocol does.  With every first frame 0 this is summarize_scores(J, F) field for field.  `frames` is the range
    of an object given on frame 0, obj_frames[k - 1] the range of object k; an empty range raises RmemError naming the object."""
    J, F = np.asarray(J, dtype=np.float64), np.asarray(F, dtype=np.float64)
    n, num_objs = J.shape
    first = [int(t) for t in first_frames]
    if len(first) != num_objs or num_objs == 0:
        raise _lib.RmemError(f'score_annotated_clip: {len(first)} first frames for {num_objs} objects')
    if not 0.0 < tail <= 1.0:
        raise _lib.RmemError(f'score_annotated_clip: tail must be in (0, 1] (got {tail})')
    sels = [np.arange(t + 1, n - 1) for t in first]
    for k, (t, sel) in enumerate(zip(first, sels), start=1):
        if t < 0 or sel.size == 0:
            raise _lib.RmemError(f'score_annotated_clip: object {k} first appears on frame {t} of {n}: no frame to score it on '
                                 f'(frames {t + 1}..{n - 2})')
    if not any(first):
        score = summarize_scores(J, F, slice(1, -1), tail)
        score.obj_frames = sels
        return score
    js = np.array([sequence_statistics(J[sel, o]) for o, sel in enumerate(sels)])
    fs = np.array([sequence_statistics(F[sel, o]) for o, sel in enumerate(sels)])
    jt = np.array([J[sel[int(sel.size * (1.0 - tail)):], o].mean() for o, sel in enumerate(sels)])
    return ClipScore(J=J, F=F, frames=np.arange(n)[1:-1], J_obj_mean=js[:, 0], J_obj_recall=js[:, 1], J_obj_decay=js[:, 2],
                     F_obj_mean=fs[:, 0], F_obj_recall=fs[:, 1], F_obj_decay=fs[:, 2], J_obj_tail=jt, J_mean=float(js[:, 0].mean()),
                     J_recall=float(js[:, 1].mean()), J_decay=float(js[:, 2].mean()), F_mean=float(fs[:, 0].mean()),
                     F_recall=float(fs[:, 1].mean()), F_decay=float(fs[:, 2].mean()),
                     JF_mean=float(0.5 * (js[:, 0].mean() + fs[:, 0].mean())), J_tail=float(jt.mean()), obj_frames=sels)


def score_annotated_clip(pred_u8: torch.Tensor, gt_u8: torch.Tensor, protocol, tail: float = 0.25, bound_th: float = 0.008) -> ClipScore:
    """score_clip for an annotation-driven run: pred_u8 [n, H, W] in squeezed ids (what run_annotated_clips yields), gt_u8 the
    full ground-truth stack in ORIGINAL ids, protocol the clip's protocol.ClipProtocol.  The ground truth is squeezed on the device
    (protocol.remap_labels with lut_all; void stays void), one clip_counts call and one device-to-host copy follow, and every
    object is summarised over its own frames (summarize_scores_per_object): an object that enters at frame t is not scored
    against an empty ground truth on frames 1 .. t."""
    from .protocol import remap_labels
    pred, gt = _label_stacks(pred_u8, gt_u8, 'score_annotated_clip')
    if not 1 <= protocol.num_objs <= 31:
        raise _lib.RmemError(f'score_annotated_clip: num_objs must be in 1..31 (got {protocol.num_objs})')
    gt = remap_labels(gt, protocol.lut_all)
    J, F = scores_from_counts(clip_counts(pred, gt, protocol.num_objs + 1, 255, bound_th).cpu().numpy())
    return summarize_scores_per_object(J[:, 1:], F[:, 1:], protocol.first_frame, tail)


def object_boxes(labels_u8: torch.Tensor, num_objs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tracks for box-based consumers: (area int32 [n, num_objs], box int32 [n, num_objs, 4] = xmin, ymin, xmax, ymax) of ids
    1..num_objs in a predicted stack [n, H, W] (uint8, device); an object absent from a frame has area 0 and box (W, H, -1, -1).
    One census call on the current stream (protocol.label_census), no host sync."""
    from .protocol import label_census
    if not 1 <= int(num_objs) <= 255:
        raise _lib.RmemError(f'object_boxes: num_objs must be in 1..255 (got {num_objs})')
    area, box = label_census(labels_u8)
    return area[:, 1:int(num_objs) + 1], box[:, 1:int(num_objs) + 1]


def object_shapes(labels_u8: torch.Tensor, num_objs: int, squeeze_idx: Optional[Sequence[int]] = None) -> List[Dict]:
    """What shape every object has: per frame of a predicted stack [n, H, W] (uint8, device) {object id: props} for the ids
    1..num_objs the frame holds (squeeze_idx: keyed by squeeze_idx[id], save_masks' un-squeeze) -- area, centroid, central moments,
    orientation, axis lengths, eccentricity, convex hull, solidity, extent, Feret diameter and the minimum-area rectangle;
    shapes.props_from_tables lists them.  Moments and hulls come from the device (shapes.region_props); the current stream, one
    4-byte readback and one of the tables."""
    from .shapes import region_props
    return region_props(labels_u8, num_objs, squeeze_idx)


def object_centroids(labels_u8: torch.Tensor, num_objs: int) -> np.ndarray:
    """Centre tracks (OTB / LaSOT centre location error): float64 [n, num_objs, 2] = (x, y) of the centroid of the ids 1..num_objs in
    a predicted stack [n, H, W] (uint8, device), in pixel-index coordinates, NaN where a frame lacks the object.  One call of
    shapes.label_moments on the current stream and one readback of its table; nothing else is computed."""
    from .shapes import label_moments
    K = _labels.int_in('object_centroids', 'num_objs', num_objs, 1, 255)
    m = label_moments(labels_u8)[:, 1:K + 1, :3].cpu().numpy().astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(m[..., :1] > 0, m[..., 1:3] / m[..., :1], np.nan)


def rotated_boxes(labels_u8: torch.Tensor, num_objs: int) -> np.ndarray:
    """VOT's rotated boxes from masks: float64 [n, num_objs, 8] = x1, y1, ..., x4, y4 of the minimum-area rectangle around the ids
    1..num_objs in a predicted stack [n, H, W] (uint8, device), in pixel-corner coordinates (a single pixel at (x, y) has the box
    x..x + 1, y..y + 1), NaN where a frame lacks the object.  shapes.region_props' min_rect."""
    K = _labels.int_in('rotated_boxes', 'num_objs', num_objs, 1, 255)
    frames = object_shapes(labels_u8, K)
    out = np.full((len(frames), K, 8), np.nan, dtype=np.float64)
    for f, fr in enumerate(frames):
        for v, props in fr.items():
            out[f, v - 1] = props['min_rect'].reshape(-1)
    return out


def clean_masks(labels_u8: torch.Tensor, fill_holes: int = 0, remove_specks: int = 0, keep_largest: bool = False,
                connectivity: int = 8) -> torch.Tensor:
    """The usual clean-up of delivered labels before they are written or scored, on the device: a new uint8 stack like labels_u8
    ([n, H, W] or [H, W], device) in which holes of up to fill_holes pixels wholly inside one object are filled with it, pieces of
    up to remove_specks pixels are dropped and, with keep_largest, only the largest piece of every object stays (a dropped piece
    becomes the one value around it, or background) -- components.clean_labels, whose docstring has the rule; every decision is
    taken from the input's connected components, frame by frame.  Something the caller applies to the labels a run delivered:
    nothing here feeds it back into a memory bank.  The current stream; one 4-byte readback at the end."""
    from .components import clean_labels
    return clean_labels(labels_u8, max_hole_area=fill_holes, max_sprinkle_area=remove_specks, keep_largest=keep_largest,
                        connectivity=connectivity)


def object_fragments(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8) -> torch.Tensor:
    """int32 [n, num_objs + 1] on the device: into how many connected pieces every value 0..num_objs of a predicted stack
    [n, H, W] (uint8, device) falls on every frame -- 1 for a mask in one piece, 0 for an absent object
    (components.object_fragments).  The current stream, no host sync."""
    from .components import object_fragments as fragments
    return fragments(labels_u8, num_objs, connectivity)


def remove_flicker(labels_u8: torch.Tensor, min_frames: int = 3, fill_frames: int = 0, connectivity: int = 8,
                   temporal: int = 1) -> torch.Tensor:
    """Delivered labels without their flicker, on the device: a new uint8 stack like labels_u8 ([n, H, W], device) in which every
    space-time piece of an object that begins after frame 0, ends before the last frame and lives for fewer than min_frames
    frames is replaced by the one value around it (else background) -- the false blob of a frame or two, whatever its area, which
    clean_masks(remove_specks=...) cannot tell from a small real object -- and, with fill_frames, a gap inside one object that is
    open for at most fill_frames frames is filled with it (tubes.clean_tubes, whose docstring has the rule).  The stack is taken
    whole.  Like clean_masks, something the caller applies to the labels a run delivered: nothing here feeds it back into a memory
    bank.  The current stream; one 8-byte readback."""
    from .tubes import clean_tubes
    return clean_tubes(labels_u8, min_frames=min_frames, max_hole_frames=fill_frames, connectivity=connectivity, temporal=temporal)


def object_events(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8, temporal: int = 1) -> torch.Tensor:
    """int32 [n, num_objs + 1, 4] on the device: per frame and value 0..num_objs the number of its pieces that are (born, ended,
    splitting, merging) there (tubes.piece_events).  object_fragments says that an object has 1 piece on frame 40 and 2 on frame
    41; this says whether a piece was cut in two (splitting 1 on frame 40) or an unrelated blob appeared beside it (born 1 on
    frame 41).  The current stream, no host sync."""
    from .tubes import piece_events
    K = _labels.int_in('evaluator.object_events', 'num_objs', num_objs, 1, 255)
    return piece_events(labels_u8, connectivity, temporal)[:, :K + 1].contiguous()


def object_tracks(labels_u8: torch.Tensor, num_objs: int, connectivity: int = 8, temporal: int = 1) -> Dict[int, List[Dict[str, int]]]:
    """{object id: [{'first_frame', 'last_frame', 'voxels', 'pieces', 'peak_area'}, ...]} on the host, for the ids 1..num_objs: the
    space-time pieces (tubes.tube_table) of every object, each list in order of first voxel.  One entry: the object is one track.
    Two: it left and came back, or was never in one piece.  None: it is absent.  One readback of the table."""
    from .tubes import tube_table
    K = _labels.int_in('evaluator.object_tracks', 'num_objs', num_objs, 1, 255)
    table, _ = tube_table(labels_u8, connectivity, temporal)
    tracks: Dict[int, List[Dict[str, int]]] = {k: [] for k in range(1, K + 1)}
    for first, value, voxels, pieces, f_first, f_last, _lo, _hi, _border, peak in table.cpu().tolist():
        if 1 <= value <= K:
            tracks[value].append({'first_frame': f_first, 'last_frame': f_last, 'voxels': voxels, 'pieces': pieces, 'peak_area': peak})
    return tracks


def surface_distance(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: int) -> np.ndarray:
    """float64 numpy [n, num_objs]: the Hausdorff distance in pixels between the predicted and the annotated mask of object
    1..num_objs on every frame (distance.hausdorff): 0 where both are empty, inf where exactly one is.  The third number reported
    for a segmentation next to J and F, and the one a far-away false blob shows in.  A void label is an ordinary value here.  Exact
    integer distance transforms on the device, one readback."""
    from .distance import hausdorff
    return hausdorff(pred_u8, gt_u8, num_objs)


def surface_metrics(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: int, tolerances: Sequence[float] = (1.0, 2.0),
                    percentile: float = 95.0, pooled: bool = True) -> Dict[str, np.ndarray]:
    """dict of float64 numpy arrays [n, num_objs] ('nsd': [n, num_objs, len(tolerances)]): the robust companions of
    surface_distance, measured surface to surface between the predicted and the annotated mask of object 1..num_objs on every frame
    (surface.surface_metrics): 'hd' the Hausdorff distance of the two surfaces, 'hd95' its 95th-percentile form (one stray pixel
    does not decide it), 'assd' the average symmetric surface distance, 'nsd' the surface Dice at each tolerance in pixels.  Both
    surfaces empty: distances 0, nsd 1; exactly one: inf and 0.  Integer census on the device, one readback."""
    from .surface import surface_metrics as _metrics
    return _metrics(pred_u8, gt_u8, num_objs, tolerances, percentile, pooled)


def next_clicks(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: int) -> np.ndarray:
    """int32 numpy [n, num_objs, 4]: (y, x, positive, d2) of the next corrective click of an interactive protocol for object
    1..num_objs on every frame; (-1, -1, 0, 0) where the object has no error on the frame.  The DEEPEST-POINT rule: per object the
    error stack E is 0 where pred and gt agree on "is object i", 1 on a false negative (gt == i, pred != i) and 2 on a false
    positive; d2 = distance.label_edt(E, border=True) is every error pixel's squared distance to the nearest pixel of another
    kind, the outside of the frame included; the click goes to the peak of the kind with the larger d2 (distance.peaks: the first
    pixel in raster order among equals), positive = 1 for a false-negative peak, and to the false positive on equal depth.
    RITM-style simulators vary this rule (the peak of an inner mask at half the maximum, a random choice among equals); this is
    the plain form and the steps above are its specification.  A void label is an ordinary value.  E is built with torch ops on
    the device; one transform and one peaks call per object, one readback in all."""
    from .distance import label_edt, peaks
    what = 'evaluator.next_clicks'
    K = _labels.int_in(what, 'num_objs', num_objs, 1, 255)
    pred, gt = _labels.stack_pair(what, pred_u8, gt_u8, ('pred', 'gt'))
    n, H, W = pred.shape
    tops = torch.empty(n, K, 2, 2, dtype=torch.int32, device=pred.device)
    d2 = torch.empty(n, H, W, dtype=torch.int32, device=pred.device)
    for i in range(1, K + 1):
        p, g = pred == i, gt == i
        E = (g & ~p).to(torch.uint8) + (p & ~g).to(torch.uint8) * 2
        label_edt(E, border=True, out=d2)
        tops[:, i - 1] = peaks(d2, E)[:, 1:3]
    t = tops.cpu().numpy().astype(np.int64)                           # [n, K, kind (fn, fp), (d2, index)]
    fn, fp = t[:, :, 0], t[:, :, 1]
    positive = fn[..., 0] > fp[..., 0]
    best = np.where(positive[..., None], fn, fp)
    none = best[..., 0] < 0
    out = np.stack([best[..., 1] // W, best[..., 1] % W, positive.astype(np.int64), best[..., 0]], axis=-1)
    out[none] = (-1, -1, 0, 0)
    return out.astype(np.int32)


def next_scribbles(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: int, min_depth2: int = 4) -> List[Dict[int, dict]]:
    """The scribble twin of next_clicks: per frame {object id: {'positive': bool, 'path': int32 numpy [k, 2] of (y, x), 'depth2':
    int}} for the objects 1..num_objs that get a corrective scribble; an object without one is absent.  All objects are handled in
    TWO stacks: FN = gt where pred != gt, else 0 (the false negatives of object v carry value v) and FP = pred where pred != gt,
    else 0, values above num_objs zeroed in both.  Per stack: d2 = distance.label_edt(stack, border=True), skeleton.thin,
    skeleton.pixels(skeleton, samples=d2), then one readback of the lists.  Per frame and object the kind whose deepest skeleton
    pixel has the larger d2 is taken, the false positive on equal depth (as next_clicks does); below min_depth2 there is no
    scribble; otherwise the 8-connected skeleton component that holds the deepest pixel (the first in raster order among equals)
    goes through skeleton.longest_path.  positive = True for a false negative.  The DAVIS interactive robot's own choices (an
    opening first, Bezier smoothing, a sampling of the path) are not reproduced; these steps are the specification.  A void label
    is an ordinary value."""
    from .distance import label_edt
    from .skeleton import component, longest_path, pixels, thin
    what = 'evaluator.next_scribbles'
    K = _labels.int_in(what, 'num_objs', num_objs, 1, 255)
    D = _labels.int_in(what, 'min_depth2', min_depth2, 0, 2 ** 31 - 1)
    pred, gt = _labels.stack_pair(what, pred_u8, gt_u8, ('pred', 'gt'))
    n = pred.shape[0]
    differ = pred != gt
    lists = []
    for src in (gt, pred):                                            # false negatives, false positives
        stack = torch.where(differ & (src <= K), src, torch.zeros_like(src))
        e, _, s = pixels(thin(stack), samples=label_edt(stack, border=True))
        lists.append((e, s))
    lists = [(e.cpu().numpy(), s.cpu().numpy()) for e, s in lists]
    out: List[Dict[int, dict]] = [{} for _ in range(n)]
    best: Dict[Tuple[int, int], tuple] = {}
    for positive, (e, s) in ((True, lists[0]), (False, lists[1])):
        if e.shape[0] == 0:
            continue
        key = e[:, 0].astype(np.int64) * 256 + e[:, 3]
        order = np.argsort(key, kind='stable')                       # raster order kept inside every (frame, value)
        cuts = np.nonzero(np.diff(key[order]))[0] + 1
        for rows in np.split(order, cuts):
            k = int(np.argmax(s[rows]))                               # the first in raster order among equals
            depth, fv = int(s[rows[k]]), (int(e[rows[0], 0]), int(e[rows[0], 3]))
            if fv not in best or depth >= best[fv][0]:                # the false positive on equal depth
                best[fv] = (depth, positive, e[rows][:, 1:3], k)
    for (f, v), (depth, positive, yx, k) in sorted(best.items()):
        if depth >= D:
            out[f][v] = {'positive': positive, 'path': longest_path(yx[component(yx, k)]), 'depth2': depth}
    return out


def expand_masks(labels_u8: torch.Tensor, distance: float, void: Optional[int] = None) -> torch.Tensor:
    """A new uint8 stack like labels_u8 ([n, H, W] or [H, W], device) in which every background pixel (value 0) within `distance`
    pixels of an object has taken the nearest object's value -- skimage.segmentation.expand_labels' rule: objects grow without
    ever overwriting one another, which closes the one-pixel gaps polygon and run-length annotations leave between touching
    objects and builds tolerance bands.  Between equally near objects the pixel goes to the one whose nearest pixel comes first
    in raster order (distance.nearest's rule; scikit-image takes whichever its host transform returns).  distance = r means squared distances
    up to int(r * r).  void (1..255), if given, is neither filled nor spread.  distance.grow; the current stream, no host sync."""
    from .distance import grow
    what = 'evaluator.expand_masks'
    if distance is None:
        raise _lib.RmemError(f'{what}: distance must be a finite number that is not negative (got None)')
    sites = set(range(1, 256))
    if void is not None:
        sites.discard(_labels.int_in(what, 'void', void, 1, 255, 'None or an integer in'))
    return grow(labels_u8, fill=(0,), sites=sorted(sites), max_distance=distance)


def fill_void(labels_u8: torch.Tensor, void: int = 255, max_distance: Optional[float] = None) -> torch.Tensor:
    """A new uint8 stack like labels_u8 in which every pixel of value `void` (the 255 DAVIS-2016 / VOC-style annotations put on
    uncertain boundary pixels, which png.decode_label_stack delivers as it is) has become the nearest other value, background
    included, ties to the site that comes first in raster order: what a first-frame label or a ground truth for score_clip needs.
    max_distance: void pixels farther than that from every other value stay void; a frame of nothing but void stays as it is.
    distance.grow; the current stream, no host sync."""
    from .distance import grow
    return grow(labels_u8, fill=(_labels.int_in('evaluator.fill_void', 'void', void, 0, 255),), sites=None, max_distance=max_distance)


def labels_from_seeds(seeds_u8: torch.Tensor, background: Optional[int] = None, max_distance: Optional[float] = None) -> torch.Tensor:
    """A new uint8 label stack from a sparse seed stack (clicks, scribbles: next_clicks, next_scribbles): every pixel of value 0
    takes the value of the nearest seed (a non-zero pixel), ties to the seed that comes first in raster order -- the nearest-seed
    partition, the baseline rule of interactive protocols.  background (1..255), if given, is the value of NEGATIVE seeds: they
    claim their region like any other and are then written as 0 (a masked_fill on the device).  max_distance: pixels farther than
    that from every seed stay 0.  A frame without seeds is returned as it is.  distance.grow; the current stream, no host sync."""
    from .distance import grow
    what = 'evaluator.labels_from_seeds'
    b = None if background is None else _labels.int_in(what, 'background', background, 1, 255, 'None or an integer in')
    out = grow(seeds_u8, fill=(0,), sites=None, max_distance=max_distance)
    return out if b is None else out.masked_fill_(out == b, 0)


def labels_from_seeds_geodesic(seeds_u8: torch.Tensor, image_u8: torch.Tensor, spatial: int = 1, colour: int = 1,
                               background: Optional[int] = None, max_cost: Optional[int] = None) -> torch.Tensor:
    """labels_from_seeds with the image-aware partition: every pixel of value 0 takes the value of the seed with the CHEAPEST PATH
    to it through the frame (distance.geodesic_grow: a step costs spatial * (5 or 7) + colour * the summed absolute difference of
    the two pixels), ties to the seed that comes first in raster order.  A click inside an object claims the object up to its
    edge, not everything nearer to it than to the next click.  image_u8: the frames, uint8 on the seeds' device, the seeds' shape
    (grey) or that with 1 or 3 interleaved channels after it.  background: as labels_from_seeds, negative seeds claim their region
    and are then written as 0.  max_cost: pixels no seed reaches within it stay 0.  A frame without seeds is returned as it is."""
    from .distance import geodesic_grow
    what = 'evaluator.labels_from_seeds_geodesic'
    b = None if background is None else _labels.int_in(what, 'background', background, 1, 255, 'None or an integer in')
    out = geodesic_grow(seeds_u8, image_u8, fill=(0,), sites=None, spatial=spatial, colour=colour, max_cost=max_cost)
    return out if b is None else out.masked_fill_(out == b, 0)


def fill_void_geodesic(labels_u8: torch.Tensor, image_u8: torch.Tensor, void: int = 255, spatial: int = 1, colour: int = 1,
                       max_cost: Optional[int] = None) -> torch.Tensor:
    """fill_void's image-aware twin: every pixel of value `void` becomes the other value, background included, with the cheapest
    path to it through the frame (distance.geodesic_grow), so a void rim round an object is split along the frame's edge inside
    it, not down its middle.  max_cost: void pixels nothing reaches within it stay void; a frame of nothing but void stays as it
    is."""
    from .distance import geodesic_grow
    v = _labels.int_in('evaluator.fill_void_geodesic', 'void', void, 0, 255)
    return geodesic_grow(labels_u8, image_u8, fill=(v,), sites=None, spatial=spatial, colour=colour, max_cost=max_cost)


def snap_masks(labels_u8: torch.Tensor, image_u8: torch.Tensor, band: float, unknown: int = 255, keep_thin: bool = True, spatial: int = 1,
               colour: int = 1) -> torch.Tensor:
    """A new uint8 stack like labels_u8 whose boundaries have moved to the frame's edges within a band: every pixel whose squared
    distance to the nearest pixel of another value (distance.label_edt(labels, border=False)) is at most int(band^2) becomes
    `unknown`, pixels already `unknown` stay so, and distance.geodesic_grow(fill=(unknown,), sites=None) regrows the band from what
    is left.  keep_thin: the pixels of skeleton.thin(labels) keep their value, so an object thinner than the band keeps a core
    and does not vanish.  band: 1..63 pixels.  Like clean_masks, something the caller applies to the labels a run delivered:
    nothing here feeds it back into a memory bank.  image_u8, spatial, colour: as distance.geodesic_grow."""
    from .distance import geodesic_grow, label_edt
    from .skeleton import thin
    what = 'evaluator.snap_masks'
    if isinstance(band, bool) or not isinstance(band, (int, float, np.integer, np.floating)) or not 1 <= band <= 63:
        raise _lib.RmemError(f'{what}: band must be a number in 1..63 (got {band!r})')
    u = _labels.int_in(what, 'unknown', unknown, 0, 255)
    a = _labels.stack(what, labels_u8)
    near = label_edt(a, border=False) <= int(float(band) * float(band))
    if keep_thin:
        near &= thin(a) == 0
    cut = a.masked_fill(near, u).view(labels_u8.shape)
    return geodesic_grow(cut, image_u8, fill=(u,), sites=None, spatial=spatial, colour=colour)


def _seed_value(what: str, obj: int, positive: bool, background: Optional[int]) -> int:
    if positive:
        return _labels.int_in(what, 'an object id', obj, 1, 255)
    if background is None:
        raise _lib.RmemError(f'{what}: object {obj} has a negative seed: give background, labels_from_seeds\' value for negative seeds')
    return background


def seeds_from_scribbles(scribbles: Sequence[Dict[int, dict]], size: Tuple[int, int], device, radius: float = 0,
                         background: Optional[int] = None) -> torch.Tensor:
    """The uint8 [n, H, W] seed stack on `device` of next_scribbles' own output (per frame {object id: {'positive', 'path':
    [k, 2] of (y, x), ...}}): what labels_from_seeds takes.  A positive scribble of object v draws value v, a negative one draws
    `background` (1..255, labels_from_seeds' value for negative seeds; a negative scribble without it is refused).  Within a frame
    the strokes are drawn in ascending object id, so where two cross the larger id shows.  radius (pixels, 0..256): 0 draws the
    path's own pixels, anything larger a round brush.  Drawn on the device (strokes.draw_label_stack): only the paths cross to it."""
    from . import strokes
    what = 'evaluator.seeds_from_scribbles'
    b = None if background is None else _labels.int_in(what, 'background', background, 1, 255, 'None or an integer in')
    frames = []
    for fr in scribbles:
        listed = []
        for v in sorted(fr):
            path = np.asarray(fr[v]['path'], dtype=np.float64).reshape(-1, 2)[:, ::-1]          # (y, x) -> (x, y)
            listed.append({'value': _seed_value(what, v, bool(fr[v]['positive']), b), 'path': path, 'radius': radius})
        frames.append(listed)
    return strokes.draw_label_stack(frames, size, device)


def seeds_from_clicks(clicks, size: Tuple[int, int], device, radius: float = 0, background: Optional[int] = None) -> torch.Tensor:
    """seeds_from_scribbles' twin for next_clicks' int32 [n, num_objs, 4] of (y, x, positive, d2): a dot (radius 0) or a disc per
    click, value = the object id for a positive click and `background` for a negative one; rows of (-1, -1, 0, 0) draw nothing."""
    from . import strokes
    what = 'evaluator.seeds_from_clicks'
    b = None if background is None else _labels.int_in(what, 'background', background, 1, 255, 'None or an integer in')
    c = np.asarray(clicks)
    if c.ndim != 3 or c.shape[2] != 4 or c.shape[0] < 1 or not np.issubdtype(c.dtype, np.integer):
        raise _lib.RmemError(f'{what}: clicks must be an integer array [n, num_objs, 4] of (y, x, positive, d2) (got {c.dtype} {c.shape})')
    frames = [[{'value': _seed_value(what, i + 1, bool(row[2]), b), 'path': [(int(row[1]), int(row[0]))], 'radius': radius}
               for i, row in enumerate(fr) if row[0] >= 0 and row[1] >= 0] for fr in c]
    return strokes.draw_label_stack(frames, size, device)


def labels_from_scribbles(doc: Dict, size: Tuple[int, int], device, radius: float = 0, ids: Optional[Sequence] = None) -> torch.Tensor:
    """The uint8 [n, H, W] stack of a DAVIS-interactive scribble document, {'scribbles': [[{'path': [[x, y], ...], 'object_id': k,
    ...}, ...] per frame]} with coordinates in [0, 1]: points are scaled by (W - 1, H - 1) and truncated to integer pixels, as
    the toolkit does; a scribble draws its object_id, or with ids the position of its object_id in ids plus one (scribbles of
    other objects are left out), in the file's order.  radius as in seeds_from_scribbles.  The toolkit's Bezier smoothing and its
    Bresenham lines are not reproduced: strokes.py's hairline rule is the specification.  Feeds labels_from_seeds, or with a brush
    an add_reference_frame."""
    from . import strokes
    what = 'evaluator.labels_from_scribbles'
    if not isinstance(doc, dict) or not isinstance(doc.get('scribbles'), (list, tuple)):
        raise _lib.RmemError(f'{what}: doc must be a dict whose \'scribbles\' lists the scribbles of every frame')
    H, W = int(size[0]), int(size[1])
    value = None if ids is None else {k: i + 1 for i, k in enumerate(ids)}
    frames = []
    for f, fr in enumerate(doc['scribbles']):
        listed = []
        for s in fr:
            if not isinstance(s, dict) or 'path' not in s or 'object_id' not in s:
                raise _lib.RmemError(f'{what}: frame {f}: a scribble is a dict with \'path\' and \'object_id\'')
            k = s['object_id']
            if value is not None and k not in value:
                continue
            p = np.asarray(s['path'], dtype=np.float64).reshape(-1, 2)
            if not ((p >= 0) & (p <= 1)).all():                       # also every NaN
                raise _lib.RmemError(f'{what}: frame {f}, object {k}: path coordinates must lie in [0, 1]')
            if len(p):
                listed.append({'value': k if value is None else value[k], 'path': np.trunc(p * (W - 1, H - 1)), 'radius': radius})
        frames.append(listed)
    return strokes.draw_label_stack(frames, (H, W), device)


def relabel_to_match(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_pred: int, num_gt: int):
    """Predictions whose ids are not the annotation's (another run, another squeeze order, an identity-free protocol) in the
    annotation's ids: (pred relabelled uint8 like pred_u8, mapping {pred id: gt id}, track IoU float64 [num_pred, num_gt]).
    pairs.pair_census of the two stacks ([n, H, W] or [H, W] uint8, device; pred ids 1..num_pred, gt ids 1..num_gt, gt may carry
    void), one readback, pairs.track_iou, pairs.assign on it (one-to-one, largest total track IoU, pairs that never overlap left
    out), one protocol.remap_labels launch.  Predicted ids without a partner get num_gt + 1, num_gt + 2, ... in ascending order
    (RmemError if those pass 255); predicted values above num_pred become background.  The returned stack goes into score_clip /
    score_annotated_clip unchanged.  The assignment is on track IoU alone: DAVIS's unsupervised matching, on the mean of J and F
    of every pair, is another rule (score_unsupervised_clip)."""
    from . import pairs
    from .protocol import remap_labels
    census = pairs.pair_census(pred_u8, gt_u8, num_pred, num_gt)
    iou = pairs.track_iou(census.cpu().numpy())
    mapping = {i + 1: j + 1 for i, j in pairs.assign(iou)}
    spare = int(num_gt)
    for i in range(1, int(num_pred) + 1):
        if i not in mapping:
            spare += 1
            mapping[i] = spare
    if spare > 255:
        raise _lib.RmemError(f'relabel_to_match: {spare - int(num_gt)} predicted ids without a partner do not fit above '
                             f'{num_gt} annotated ids (ids end at 255)')
    lut = np.zeros(256, dtype=np.uint8)
    for i, j in mapping.items():
        lut[i] = j
    return remap_labels(pred_u8, lut), dict(sorted(mapping.items())), iou


@dataclass
class ObjectIdentity:
    """identity_report's entry for one object i.  J_own: per-frame J of predicted i against annotated i [n] (empty against empty
    is 1, as db_eval_iou has it); rival: the annotated id j != i with the largest track IoU with predicted i (the smallest such j
    on a tie), None when predicted i overlaps no other object; rival_iou: that track IoU (0.0 without a rival); switch_frames: the
    frames on which predicted i is not empty and overlaps some annotated j != i with a higher IoU than annotated i."""
    J_own: np.ndarray
    rival: Optional[int]
    rival_iou: float
    switch_frames: List[int]


def identity_report(pred_u8: torch.Tensor, gt_u8: torch.Tensor, num_objs: int, void_label: Optional[int] = 255) -> Dict[int, ObjectIdentity]:
    """Where did the mask go?  For a run whose ids are aligned with the annotation's ([n, H, W] or [H, W] uint8 device stacks,
    objects 1..num_objs, up to 255 of them where score_clip stops at 31): {i: ObjectIdentity}.  J per object going to zero does
    not tell an identity swap from a lost object; the overlap of predicted i with annotated j != i does.  One pairs.pair_census
    launch and one readback.  void_label (default 255) must lie above num_objs: annotated pixels of values above num_objs, void
    among them, count nowhere; None counts every pixel."""
    from . import pairs
    if void_label is not None and isinstance(num_objs, (int, np.integer)) and int(void_label) <= int(num_objs):
        raise _lib.RmemError(f'identity_report: void_label {void_label} must lie above num_objs {num_objs} (or be None)')
    census = pairs.pair_census(pred_u8, gt_u8, num_objs, num_objs).cpu().numpy()
    drop = void_label is not None
    iou, inter, union = pairs.pair_iou(census, drop_other_b=drop)
    track = pairs.track_iou(census, drop_other_b=drop)
    n, K = iou.shape[0], int(num_objs)
    c = census[:, :, :-1] if drop else census
    pred_area = c.sum(axis=2)[:, 1:K + 1]                          # [n, K]: predicted i on pixels that count
    diag = np.arange(K)
    own_u = union[:, diag, diag]
    J_own = np.where(own_u == 0, 1.0, inter[:, diag, diag] / np.maximum(own_u, 1))
    own = np.where(own_u == 0, 0.0, J_own)
    others = np.where(np.isnan(iou), 0.0, iou)
    others[:, diag, diag] = -1.0
    rivals = track.copy()
    rivals[diag, diag] = 0.0
    report = {}
    for k in range(K):
        j = int(np.argmax(rivals[k]))
        has = rivals[k, j] > 0.0
        switched = (pred_area[:, k] > 0) & (others[:, k].max(axis=1) > own[:, k]) if K > 1 else np.zeros(n, dtype=bool)
        report[k + 1] = ObjectIdentity(J_own=J_own[:, k], rival=j + 1 if has else None, rival_iou=float(rivals[k, j]) if has else 0.0,
                                       switch_frames=np.nonzero(switched)[0].tolist())
    return report


def frames_from_jpegs(paths_or_bytes: Sequence, device, scale: float = 1.0) -> torch.Tensor:
    """A clip's JPEG files (paths or bytes, one size) -> fp32 [n, 3, H, W] normalised frames at the network size
    synth.network_size(h, w, scale=scale): GPU decode (rmem_jpeg_decode_batch, jpeg.CHUNK frames per call) then bicubic resize + normalise
    (rmem_ingest_rgb8), the input SequenceEvaluator.run takes."""
    from .frame_feed import FrameFeed
    from .jpeg import CHUNK, JpegClip
    from .synth import network_size
    device = torch.device(device)
    datas = []
    for p in paths_or_bytes:
        if isinstance(p, (bytes, bytearray, memoryview)):
            datas.append(bytes(p))
        else:
            with open(p, 'rb') as f:
                datas.append(f.read())
    clip = JpegClip(datas)
    n, (hs, ws) = len(clip), clip.sizes[0]
    H, W = network_size(hs, ws, scale=scale)
    out = torch.empty(n, 3, H, W, dtype=torch.float32, device=device)
    rgb = torch.empty(min(n, CHUNK), hs, ws, 3, dtype=torch.uint8, device=device)     # one chunk of decoded frames at a time
    stream = torch.cuda.current_stream(device).cuda_stream
    feed = FrameFeed(device)
    for k in range(0, n, CHUNK):
        feed.ingest([(clip, k, min(CHUNK, n - k), rgb, out[k:])], stream)
    clip.check(device, stream=stream)
    return out


def labels_from_pngs(paths_or_bytes: Sequence, device, lut=None) -> torch.Tensor:
    """A clip's annotation files (paths or bytes, one size; indexed PNGs, or 8-bit grey ones such as 0 / 255 masks with
    lut[255] = 1) -> uint8 [n, H, W] label maps on the device, decoded there (png.decode_label_stack): the ground truth
    score_clip takes, and with gt[0].float()[None, None] the first-frame mask of a run."""
    from . import png
    return png.decode_label_stack(paths_or_bytes, device, lut)


def labels_from_rles(frames: Sequence[Dict], size: Tuple[int, int], device, ids: Optional[Sequence] = None):
    """A clip's run-length annotations (BURST / TAO-VOS, YouTube-VIS, SA-V: frames[f] = {track id: {'size': [H, W], 'counts':
    bytes, str or the uncompressed list}}) -> (uint8 [n, H, W] label maps on the device, ids): track ids[i] is label value i + 1,
    ids defaults to the sorted union of the keys; tracks not in ids are left out.  Decoded on the device (rle.decode_label_stack):
    only the strings cross to it.  The stack feeds protocol.clip_protocol, run_annotated_clips, score_clip and
    score_annotated_clip exactly as labels_from_pngs' does.  More than 255 tracks raise RmemError."""
    from . import rle
    ids = sorted({k for fr in frames for k in fr}) if ids is None else list(ids)
    if len(ids) > 255:
        raise _lib.RmemError(f'labels_from_rles: {len(ids)} tracks (at most 255 fit one uint8 label stack)')
    value = {k: i + 1 for i, k in enumerate(ids)}
    listed = [[(value[k], r) for k, r in fr.items() if k in value] for fr in frames]
    return rle.decode_label_stack(listed, size, device), ids


def labels_from_polygons(frames: Sequence[Dict], size: Tuple[int, int], device, ids: Optional[Sequence] = None):
    """labels_from_rles' twin for polygon tracks (CVAT, Labelme, COCO `segmentation` lists: frames[f] = {track id: shape}, a shape
    in any form polygons.PackedPolygons takes) -> (uint8 [n, H, W] label maps on the device, ids): track ids[i] is label value
    i + 1, ids defaults to the sorted union of the keys; tracks not in ids are left out.  Filled on the device
    (polygons.fill_label_stack: the even-odd rule at pixel centres, not pycocotools' frPoly): only the edges cross to it.  The stack
    feeds protocol.clip_protocol, run_annotated_clips, score_clip and score_annotated_clip exactly as labels_from_pngs' does.
    More than 255 tracks raise RmemError."""
    from . import polygons
    ids = sorted({k for fr in frames for k in fr}) if ids is None else list(ids)
    if len(ids) > 255:
        raise _lib.RmemError(f'labels_from_polygons: {len(ids)} tracks (at most 255 fit one uint8 label stack)')
    value = {k: i + 1 for i, k in enumerate(ids)}
    listed = [[(value[k], s) for k, s in fr.items() if k in value] for fr in frames]
    return polygons.fill_label_stack(listed, size, device), ids


def rle_results(labels_u8: torch.Tensor, num_objs: int, squeeze_idx: Optional[Sequence[int]] = None, boxes: bool = False,
                ascii: bool = True) -> List[Dict[int, dict]]:
    """save_masks' twin for run-length submissions: per frame of a stack of device label maps ([n, H, W] or [H, W] uint8 --
    FinishedClip.labels, slot.labels[c, 1:n], run_annotated_clips' output) {object id: {'size': [H, W], 'counts': str}} for the
    objects 1..num_objs, the strings built on the device (rle.encode_label_stack).  squeeze_idx un-squeezes the keys; boxes adds
    'area' and 'bbox' = [x, y, w, h]; ascii=False keeps the counts as bytes (pycocotools' own type)."""
    from . import rle
    return rle.encode_label_stack(labels_u8, num_objs, squeeze_idx, boxes=boxes, ascii=ascii)


def polygon_results(labels_u8: torch.Tensor, num_objs: int, squeeze_idx: Optional[Sequence[int]] = None, holes: str = 'rings',
                    connectivity: int = 8, tolerance: Optional[float] = None) -> List[Dict[int, dict]]:
    """rle_results' twin for polygon consumers (COCO `segmentation` lists, CVAT / Labelme tracks): per frame of a stack of device
    label maps ([n, H, W] or [H, W] uint8) {object id: {'size': [H, W], 'segmentation': [[x0, y0, x1, y1, ...], ...], 'area': int}}
    for the objects 1..num_objs, one ring of pixel corners per connected piece, traced on the device
    (polygons.trace_label_stack); an object the frame does not hold has an empty list and area 0.  squeeze_idx un-squeezes the
    keys.  'area' is the sum of the listed rings' area2 divided by 2.
    holes='rings': a key 'holes' of the same shape lists the holes' rings (their area2 is negative, so 'area' is the pixel count).
    holes='drop': only the exteriors are listed, which FILLS every hole -- COCO's polygon list cannot express one -- and 'area'
    is the filled area; use rle_results where holes matter.
    tolerance (pixels, 0..64; None: nothing changes): the rings are simplified on the device (polygons.simplify: Douglas-Peucker,
    every dropped vertex within the tolerance of its ring; rings may then touch or cross) and degenerate ones dropped.  'area' is
    then a FLOAT, the shoelace area of the rings the entry lists: exteriors minus the listed holes under holes='rings', exteriors
    alone under 'drop' -- no longer the pixel count."""
    from . import polygons
    if holes not in ('rings', 'drop'):
        raise _lib.RmemError(f'polygon_results: holes must be \'rings\' or \'drop\' (got {holes!r})')
    if tolerance is None:
        frames = polygons.trace_label_stack(labels_u8, num_objs, connectivity, squeeze_idx, parents=True)
        return polygons.coco_polygons(frames, labels_u8.shape[-2:], holes)
    frames = polygons.trace_label_stack(labels_u8, num_objs, connectivity, squeeze_idx, parents=True, tolerance=tolerance)
    return polygons.coco_polygons(frames, labels_u8.shape[-2:], holes, simplified=True)


class SequenceEvaluator:
    """Runs one sequence through the engine(s) exactly as the reference evaluator would."""

    def __init__(self, model, gpu_id: int = 0, flip: bool = False):
        self.model, self.gpu_id, self.flip = model, gpu_id, flip
        self.cfg = model.cfg
        self.engines = []

    def _engine(self, i):
        while len(self.engines) <= i:
            e = build_engine(self.cfg.MODEL_ENGINE, phase='eval', aot_model=self.model, gpu_id=self.gpu_id,
                             long_term_mem_gap=self.cfg.TEST_LONG_TERM_MEM_GAP)
            self.engines.append(e.eval())
        return self.engines[i]

    def run(self, frames, labels: Dict[int, torch.Tensor], out_hw: Tuple[int, int]) -> List[torch.Tensor]:
        """frames: [n, 3, H, W] fp32 device (network size, normalised) or, for multi-scale testing, a list of such tensors, one
        per entry of TEST_MULTISCALE (each at its own stride-aligned size, synth.network_size(..., scale=s));
        labels: {frame index: [1,1,Ho,Wo] fp32 label map at the ORIGINAL size}; labels[0] is the first-frame annotation,
        later entries are newly appearing objects.  One engine per (scale, flip) pair (evaluator.py:342-355); their logits
        are resized to the original size, un-flipped, soft-maxed and averaged (427-438).
        Returns the uint8 label map of every frame after the first, at the original size."""
        per_scale = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        n = per_scale[0].shape[0]
        gap = clip_gap(n)
        flips = [False, True] if self.flip else [False]
        augs = [(si, fl) for si in range(len(per_scale)) for fl in flips]      # evaluator.py:342-355 order: scale outer, flip inner
        if len(augs) > 8:
            raise ValueError('at most 8 augmentations (scales x flips)')
        aflips = [fl for _, fl in augs]
        outs: List[torch.Tensor] = []

        def resized(src, size, fl):
            """(mirror along W for a flipped augmentation, then) nearest resize to `size` on the device: rmem_resize_nearest_flip_f32"""
            dst = torch.empty(*src.shape[:-2], int(size[0]), int(size[1]), dtype=torch.float32, device=src.device)
            ops.run(ops.resize_nearest_flip(src.contiguous(), dst, flip=fl))
            return dst

        def frame(a, t):
            si, fl = augs[a]
            img = per_scale[si][t:t + 1]
            return resized(img, img.shape[-2:], True) if fl else img

        for a, (si, fl) in enumerate(augs):
            e = self._engine(a)
            e.restart_engine()
            e.long_term_mem_gap = gap
            # the first frame's label is resized THEN mirrored (the data pipeline flips the resized sample,
            # dataloaders/video_transforms.py MultiRestrictSize), later labels are mirrored then resized (evaluator.py:490-522)
            lab = resized(labels[0], per_scale[si].shape[2:], False)
            if fl:
                lab = resized(lab, lab.shape[-2:], True)
            e.add_reference_frame(frame(a, 0), lab, obj_nums=[int(labels[0].max().item())], frame_step=0)
        for t in range(1, n):
            logits = [self.engines[a].match_propogate_one_frame(frame(a, t), output_size=out_hw) for a in range(len(augs))]
            label_u8, label_f, _ = tta_merge(logits, aflips)
            if t in labels:                                   # evaluator.py:484-508
                new = labels[t]
                keep = (new == 0).float()
                label_f = label_f * keep + new * (1 - keep)
                label_u8 = label_f[0, 0].to(torch.uint8)
                nobj = [int(label_f.max().item())]
                for a, (si, fl) in enumerate(augs):
                    lab = resized(label_f, self.engines[a].input_size_2d, fl)
                    self.engines[a].add_reference_frame(frame(a, t), lab, obj_nums=nobj, frame_step=t)
            else:
                for a, (si, fl) in enumerate(augs):
                    e = self.engines[a]
                    if not fl and len(e.aot_engines) == 1:
                        # the nearest resize to the network size (evaluator.py:518-522) happens inside the one-hot kernel;
                        # a fixed buffer, so the engine's prepared launch list for it is built once
                        if getattr(self, '_lab_u8', None) is None or self._lab_u8.shape != label_u8.shape:
                            self._lab_u8 = torch.empty_like(label_u8)
                        ops.copy_async(self._lab_u8, label_u8, label_u8.numel())(torch.cuda.current_stream(label_u8.device).cuda_stream)
                        e.update_memory_from_label_u8(self._lab_u8)
                    else:
                        e.update_memory(resized(label_f, e.input_size_2d, fl))
            outs.append(label_u8)
        return outs


def run_clips(model, clips, rows: int = 8, lookahead: int = 4, flip: bool = False, out_hw: Optional[Tuple[int, int]] = None):
    """A clip list of ANY lengths at group speed: one GroupEngine of ``rows`` rows and one clip_runner.RaggedGroupSlot; a clip
    moves into a row as soon as the row's clip has ended (at most ``lookahead`` - 1 frames later).  clips: an iterable of
    (clip_id, frames, first_label, new_objects) -- frames fp32 [n, 3, H, W] on the device at the network size or uint8
    [n, Hs, Ws, 3] in pinned host memory, first_label [1, 1, H, W] fp32 label map at the network size, new_objects None or
    {frame index: uint8 [Ho, Wo] device map}.  All clips share the network size.  out_hw: the size of the delivered label maps
    (default: the network size; uint8 frames: the frames' size).  flip: flip testing, ``rows`` clips and their mirrored twins in
    a group of 2 * rows.  Yields (clip_id, labels uint8 [n, Ho, Wo] on the device, row 0 zero) as clips finish, in the order they
    finish; the current stream has been made to wait for the clip's last frame, so the stack can be scored / saved right away
    while the group runs on."""
    from .clip_runner import RaggedGroupSlot
    from .networks.engines.group_engine import GroupEngine
    it = iter(clips)
    head = next(it, None)
    if head is None:
        return
    dev = torch.device('cuda', 0)
    if out_hw is None:
        out_hw = tuple(head[1].shape[1:3]) if head[1].dtype == torch.uint8 else tuple(head[2].shape[-2:])
    eng = GroupEngine(model, 2 * rows if flip else rows, 0, lookahead=lookahead, flip_tta=flip)
    slot = RaggedGroupSlot(eng, out_hw, dev)

    def every():
        yield head
        yield from it

    for fin in slot.run(every()):
        if fin.event is not None:
            torch.cuda.current_stream(dev).wait_event(fin.event)
        yield fin.clip_id, fin.labels
    eng.synchronize()


def run_annotated_clips(model, clips, rows: int = 8, lookahead: int = 4, flip: bool = False):
    """run_clips driven by annotations.  clips: an iterable of (clip_id, frames, ann_u8, frame_index) -- frames as run_clips takes
    them, ann_u8 [m, Ho, Wo] the clip's annotation stack on the device in the files' own (sparse) ids (labels_from_pngs),
    frame_index the clip frame of every annotated row (None: row j is frame j).  Per clip: protocol.clip_protocol (ids, first
    appearances, squeeze, the first label and the overlays of objects that appear mid-clip, all on the device), the first label
    resized to the network size (nearest), then the clip goes to run_clips with out_hw = (Ho, Wo).  Yields (clip_id, labels uint8
    [n, Ho, Wo] in squeezed ids, ClipProtocol) in finish order; protocol.squeeze_idx is what save_masks takes to write the files
    in the original ids.  A clip with more than model.max_obj_num objects raises ValueError before it is submitted; the slot's own
    restrictions (new objects need fp32 device frames) surface as the slot's errors."""
    from .protocol import clip_protocol
    from .synth import network_size
    protocols = {}
    it = iter(clips)
    head = next(it, None)
    if head is None:
        return
    out_hw = tuple(int(v) for v in head[2].shape[-2:])

    def prepared():
        for clip_id, frames, ann_u8, frame_index in itertools.chain([head], it):
            if tuple(int(v) for v in ann_u8.shape[-2:]) != out_hw:
                raise ValueError(f'run_annotated_clips: clip {clip_id!r} has annotations of {tuple(ann_u8.shape[-2:])}, the run '
                                 f'delivers {out_hw}: all clips of a run share one output size')
            proto, first_u8, new_objects = clip_protocol(ann_u8, frame_index)
            if proto.num_objs > model.max_obj_num:
                raise ValueError(f'run_annotated_clips: clip {clip_id!r} has {proto.num_objs} objects, the model takes at most '
                                 f'{model.max_obj_num}')
            net = network_size(int(frames.shape[1]), int(frames.shape[2])) if frames.dtype == torch.uint8 else tuple(frames.shape[-2:])
            src = first_u8.float()[None, None].contiguous()
            first = torch.empty(1, 1, int(net[0]), int(net[1]), dtype=torch.float32, device=src.device)
            ops.run(ops.resize_nearest_flip(src, first, flip=False), torch.cuda.current_stream(src.device).cuda_stream)
            protocols[clip_id] = proto
            yield clip_id, frames, first, new_objects or None

    for clip_id, labels in run_clips(model, prepared(), rows=rows, lookahead=lookahead, flip=flip, out_hw=out_hw):
        yield clip_id, labels, protocols.pop(clip_id)


def run_group_multiscale(model, frames, first_labels, out_hw: Tuple[int, int], flip: bool = False, lookahead: int = 4,
                         new_objects=None) -> torch.Tensor:
    """Multi-scale testing (TEST_MULTISCALE, with ``flip`` also TEST_FLIP) of P clips of equal length at group speed: one GroupEngine
    per scale and one clip_runner.MultiScaleGroupSlot, whose fused merge (rmem_logits_post_ms_merge) takes the place of the
    per-augmentation full-size logit maps and rmem_tta_merge.  frames[s][c]: fp32 device tensors [n, 3, H_s, W_s], clip c at scale
    s's network size (synth.network_size(..., scale=s)); first_labels[c]: fp32 [1, 1, Ho, Wo] first-frame annotation at the
    output size; new_objects: {clip: (frame index, uint8 [Ho, Wo] device map)}.  At most 8 (scale, flip) members and 10 objects;
    SequenceEvaluator is the per-clip reference of the same protocol and takes the cases beyond.
    -> labels uint8 [P, n, Ho, Wo] on the device (row 0 zero: frame 0 is the given annotation), synchronised."""
    from .clip_runner import MultiScaleGroupSlot
    from .networks.engines.group_engine import GroupEngine
    P = len(frames[0])
    dev = frames[0][0].device
    num_objs = int(max(int(m.max().item()) for m in first_labels))
    if num_objs > model.max_obj_num:
        raise ValueError(f'run_group_multiscale: {num_objs} objects; more than {model.max_obj_num} run on SequenceEvaluator')
    engines = [GroupEngine(model, 2 * P if flip else P, dev.index or 0, lookahead=lookahead, flip_tta=flip) for _ in frames]
    slot = MultiScaleGroupSlot(engines, tuple(out_hw), dev)
    slot.start(frames, first_labels, num_objs, new_objects=new_objects)
    while not slot.done:
        slot.step()
    slot.synchronize()
    n = int(frames[0][0].shape[0])
    return slot.labels[:, :n]
