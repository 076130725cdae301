"""Planted inputs for the COCO evaluator (tmx::coco_evaluate, tmx::coco_evaluate_gpu, tmx::coco_evaluate_gpu_img and
MeanAveragePrecision), as plain data, with converters to the forms those take.

Random boxes never produce an IoU equal to a threshold, an area equal to 32^2, two ground truths at the same IoU or a
score tie across the maxDets cut; every case here plants one such rule.  Boxes are xywh with integer coordinates, so
every IoU and area is exact in fp64, and scores (except in ``score_values``) are exact in bf16, fp16 and fp32, so one
oracle result serves every score type.

``CASES[name]`` holds ``dets`` (rows ``(img, cat, box, score)``), ``gts`` (rows ``(img, cat, box, crowd, area)``; area
0 = take the box area), ``n_img``, ``iou_thrs``, ``rec_thrs`` and ``max_dets``.  ``sweep(...)`` builds the
recall-threshold sweep: one class per count of non-ignored ground truths."""
import math
from fractions import Fraction

import numpy as np
import torch

from tests.helpers import coco_oracle

IOU_THRS = np.linspace(0.5, 0.95, 10).tolist()  # pycocotools' own lists
REC_THRS = np.linspace(0.0, 1.0, 101).tolist()
assert IOU_THRS[0] == 0.5 and IOU_THRS[5] == 0.75
MAX_DETS = [1, 10, 100]
SCORE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def exact_scores(n):
    """n strictly falling scores with 8 significant bits in fp16's normal range: exact in bf16, fp16 and fp32."""
    vals = [m * 2.0 ** (e - 7) for e in range(0, -12, -1) for m in range(255, 127, -1)]
    assert n <= len(vals)
    return vals[:n]


def make_case(dets, gts, n_img, iou_thrs=None, rec_thrs=None, max_dets=None):
    """One case from integer rows; the thresholds default to COCO's."""
    return dict(dets=[(i, c, [float(v) for v in b], float(s)) for i, c, b, s in dets],
                gts=[(i, c, [float(v) for v in b], int(cr), float(ar)) for i, c, b, cr, ar in gts], n_img=n_img,
                iou_thrs=list(IOU_THRS if iou_thrs is None else iou_thrs),
                rec_thrs=list(REC_THRS if rec_thrs is None else rec_thrs),
                max_dets=list(MAX_DETS if max_dets is None else max_dets))


_case = make_case


def _build_cases():
    C = {}

    # IoU 1/2 and 3/4 exactly: matched at a threshold equal to the IoU, unmatched at the next one
    C["iou_at_threshold"] = _case(
        dets=[(0, 3, [0, 0, 2, 1], 0.5), (0, 7, [0, 0, 4, 1], 0.5)],
        gts=[(0, 3, [0, 0, 1, 1], 0, 0), (0, 7, [0, 0, 3, 1], 0, 0)], n_img=1)

    # threshold 1.0 is capped at 1 - 1e-10: an identical box still matches
    C["iou_one_capped"] = _case(dets=[(0, 1, [2, 3, 5, 7], 0.5)], gts=[(0, 1, [2, 3, 5, 7], 0, 0)], n_img=1,
                                iou_thrs=[0.5, 1.0])

    # class 1: d0 has IoU 3/4 with both ground truths and takes the later one; d1 (= g0) then takes g0 at IoU 1.  Under
    # "first wins" d0 takes g0 and d1 is left with g1 at IoU 1/2.  class 2: the same boxes with g0 medium and g1 small
    C["equal_iou_two_gts"] = _case(
        dets=[(0, 1, [0, 0, 4, 2], 0.75), (0, 1, [0, 0, 3, 2], 0.5), (0, 2, [0, 0, 4, 2], 0.75), (0, 2, [0, 0, 3, 2], 0.5)],
        gts=[(0, 1, [0, 0, 3, 2], 0, 0), (0, 1, [1, 0, 3, 2], 0, 0), (0, 2, [0, 0, 3, 2], 0, 2000), (0, 2, [1, 0, 3, 2], 0, 100)],
        n_img=1)

    # d0: IoU 3/4 with the plain ground truth, 1 with the crowd one: a TP up to 0.75, ignored above.  d1 reaches the
    # crowd box only: ignored.  d2 reaches nothing: the only FP
    C["prefers_unignored"] = _case(
        dets=[(0, 1, [0, 0, 4, 3], 0.75), (0, 1, [6, 6, 2, 2], 0.5), (0, 1, [50, 50, 4, 4], 0.25)],
        gts=[(0, 1, [0, 0, 4, 4], 0, 0), (0, 1, [0, 0, 10, 10], 1, 0)], n_img=1)

    # three detections on one crowd box (the last at intersection / detection area = 1/2 exactly; its plain IoU is 1/3),
    # and two claimants of one plain ground truth
    C["crowd_rematch"] = _case(
        dets=[(0, 1, [0, 0, 2, 2], 0.875), (0, 1, [3, 3, 2, 2], 0.75), (0, 1, [0, 0, 20, 5], 0.625),
              (0, 1, [20, 20, 4, 4], 0.5), (0, 1, [20, 20, 4, 4], 0.25), (1, 1, [0, 0, 4, 4], 0.375)],
        gts=[(0, 1, [0, 0, 10, 10], 1, 0), (0, 1, [20, 20, 4, 4], 0, 0), (1, 1, [0, 0, 4, 4], 0, 0)], n_img=2)

    # areas 1024 and 9216 belong to both adjoining ranges (closed bounds); 1023 / 1025 / 9215 / 9217 to one
    gts, dets = [], []
    for j, (box, area) in enumerate([([0, 0, 10, 10], 1024), ([0, 0, 10, 10], 9216), ([0, 0, 32, 32], 0), ([0, 0, 96, 96], 0),
                                     ([0, 0, 10, 10], 1023), ([0, 0, 10, 10], 1025), ([0, 0, 10, 10], 9215), ([0, 0, 10, 10], 9217),
                                     ([0, 0, 31, 33], 0), ([0, 0, 25, 41], 0), ([0, 0, 95, 97], 0), ([0, 0, 13, 709], 0)]):
        b = [200 * j, 0, box[2], box[3]]
        gts.append((j % 2, 1, b, 0, area))
        if j % 3 != 2:  # two of three are found
            dets.append((j % 2, 1, b, 0))
    for j, (w, h) in enumerate([(32, 32), (96, 96), (31, 33), (25, 41), (95, 97), (13, 709)]):  # unmatched
        dets.append((j % 2, 1, [200 * j, 2000, w, h], 0))
    sc = exact_scores(len(dets))
    order = [5, 0, 9, 3, 12, 7, 1, 10, 4, 13, 8, 2, 11, 6]  # found and unmatched rows interleaved in score order
    dets = [(i, c, b, sc[order.index(n)]) for n, (i, c, b, _) in enumerate(dets)]
    C["area_boundaries"] = _case(dets, gts, n_img=2)

    # medium ground truth (area 1600) matched by a small detection (area 1000, IoU 5/8): a TP in "medium".  The
    # higher-scoring unmatched small detection is ignored in "medium" and an FP in "small"
    C["unmatched_out_of_range"] = _case(
        dets=[(0, 1, [100, 100, 10, 10], 0.75), (0, 1, [0, 0, 40, 25], 0.5)],
        gts=[(0, 1, [0, 0, 40, 40], 0, 0)], n_img=1)

    # equal scores across every cut: input order decides who is kept.  image 0: TP, FP, FP | TP, FP; image 1: the two
    # 0.75 rows first, then the 0.5 rows in input order; in both the detection on the second ground truth is cut
    C["maxdet_cut_with_ties"] = _case(
        dets=[(0, 1, [0, 0, 4, 4], 0.5), (0, 1, [50, 50, 4, 4], 0.5), (0, 1, [60, 60, 4, 4], 0.5),
              (0, 1, [10, 0, 4, 4], 0.5), (0, 1, [70, 70, 4, 4], 0.5),
              (1, 1, [50, 50, 4, 4], 0.75), (1, 1, [0, 0, 4, 4], 0.5), (1, 1, [60, 60, 4, 4], 0.5),
              (1, 1, [10, 0, 4, 4], 0.5), (1, 1, [70, 70, 4, 4], 0.75)],
        gts=[(0, 1, [0, 0, 4, 4], 0, 0), (0, 1, [10, 0, 4, 4], 0, 0), (1, 1, [0, 0, 4, 4], 0, 0), (1, 1, [10, 0, 4, 4], 0, 0)],
        n_img=2, max_dets=[1, 2, 3])

    # one score in three images: FP (image 0), TP, TP in the stable order; TP, TP, FP if images merge in reverse
    C["ties_across_images"] = _case(
        dets=[(0, 1, [50, 50, 4, 4], 0.5), (1, 1, [0, 0, 4, 4], 0.5), (2, 1, [0, 0, 4, 4], 0.5), (2, 1, [0, 9, 4, 4], 0.25)],
        gts=[(0, 1, [0, 0, 4, 4], 0, 0), (1, 1, [0, 0, 4, 4], 0, 0), (2, 1, [0, 0, 4, 4], 0, 0), (2, 1, [0, 9, 4, 4], 0, 0)],
        n_img=3)

    # image 0 empty; class 1 only in ground truth; class 2 only in detections; class 3 all crowd; class 4 ordinary
    C["empty_sides"] = _case(
        dets=[(1, 2, [0, 0, 4, 4], 0.5), (2, 3, [1, 1, 2, 2], 0.5), (2, 4, [0, 0, 4, 4], 0.75)],
        gts=[(1, 1, [0, 0, 4, 4], 0, 0), (2, 3, [0, 0, 10, 10], 1, 0), (2, 4, [0, 0, 4, 4], 0, 0)], n_img=3)
    C["empty_sides_k1"] = _case(dets=[(0, 5, [0, 0, 4, 4], 0.5), (0, 5, [9, 9, 4, 4], 0.25)],
                                gts=[(0, 5, [0, 0, 4, 4], 0, 0)], n_img=1)
    C["empty_sides_no_dets"] = _case(dets=[], gts=[(0, 5, [0, 0, 4, 4], 0, 0)], n_img=1)

    # rows in score order: ignored (crowd match), FP, TP, TP: recall threshold 0 is answered at the ignored row
    C["first_row_ignored"] = _case(
        dets=[(0, 1, [1, 1, 2, 2], 0.875), (0, 1, [50, 50, 4, 4], 0.75), (0, 1, [20, 0, 4, 4], 0.625), (0, 1, [30, 0, 4, 4], 0.5)],
        gts=[(0, 1, [0, 0, 10, 10], 1, 0), (0, 1, [20, 0, 4, 4], 0, 0), (0, 1, [30, 0, 4, 4], 0, 0)], n_img=1)

    # zero-width / zero-area boxes on both sides, touching and inside others (IoU 0); a ground truth with area 0 takes
    # its box area 1600 (medium); the zero-area ground truths count as non-ignored in "all" and "small"
    C["degenerate_boxes"] = _case(
        dets=[(0, 1, [0, 0, 0, 5], 0.875), (0, 1, [3, 3, 0, 0], 0.75), (0, 1, [10, 10, 0, 4], 0.625),
              (0, 1, [20, 20, 40, 40], 0.5), (0, 1, [8, 8, 6, 6], 0.375), (0, 1, [14, 8, 3, 3], 0.25)],
        gts=[(0, 1, [0, 0, 0, 5], 0, 0), (0, 1, [3, 3, 0, 0], 0, 0), (0, 1, [8, 8, 6, 6], 0, 0), (0, 1, [20, 20, 40, 40], 0, 0),
             (0, 1, [9, 9, 0, 2], 1, 0)], n_img=1)

    # n disjoint unit ground truths per class; detection g sits on ground truth g and scores rise with g, so matching
    # starts at the highest index.  The lowest-scoring rows sit again on ground truths 31, 32, 63, 64: all FP
    dets, gts = [], []
    sc = exact_scores(80)[::-1]
    for c, n in enumerate([31, 32, 33, 64, 65]):
        for g in range(n):
            gts.append((0, 10 + c, [2 * g, 0, 1, 1], 0, 0))
            dets.append((0, 10 + c, [2 * g, 0, 1, 1], sc[10 + g]))
        for j, g in enumerate([31, 32, 63, 64]):
            if g < n:
                dets.append((0, 10 + c, [2 * g, 0, 1, 1], sc[j]))
    C["gt_word_edges"] = _case(dets, gts, n_img=1)

    # the per-image route's whole bitset: 256 ground truths of one class in one image (8 words), detections on ground
    # truths 120 .. 255 from the top down, then again on both sides of every word edge above (all FP)
    gts = [(0, 1, [2 * g, 0, 1, 1], 0, 0) for g in range(256)]
    sc = exact_scores(160)[::-1]
    dets = [(0, 1, [2 * g, 0, 1, 1], sc[g - 100]) for g in range(120, 256)]
    dets += [(0, 1, [2 * g, 0, 1, 1], sc[j]) for j, g in enumerate([127, 128, 159, 160, 191, 192, 223, 224, 255])]
    C["gt_word_edges_256"] = _case(dets, gts, n_img=1, iou_thrs=[0.5, 0.75])

    def rows(counts_d, counts_g):  # 4 classes per image; detection j on ground truth j: exact / IoU 1/2 / apart
        dets, gts = [], []
        sc = exact_scores(300)
        for i, (nd, ng) in enumerate(zip(counts_d, counts_g)):
            for j in range(ng):
                gts.append((i, j % 4, [4 * j, 0, 3, 3], int(j % 37 == 5), 0))
            for j in range(nd):
                x = 4 * j + (1 if j % 3 == 1 else 0)
                dets.append((i, j % 4, [x, 50 if j % 3 == 2 else 0, 3, 3], sc[(j * 7) % 300 // 2]))  # (score ties)
        return dets, gts

    C["image_row_limits_256"] = _case(*rows([255, 256, 3, 0], [256, 255, 0, 256]), n_img=4)
    C["image_row_limits_257_dets"] = _case(*rows([257, 5], [256, 5]), n_img=2)
    C["image_row_limits_257_gts"] = _case(*rows([256, 5], [257, 5]), n_img=2)

    # every second row is a TP (on its own ground truth), the others FP, so the score order shows in the tables.
    # 1 + 2^-9 collides with 1 in bf16, 1 + 2^-12 also in fp16; 2^-133 and 2^-24 are bf16's and fp16's smallest
    # subnormals, 2^-149 fp32's; 3.4e38 is finite in fp32 only
    vals = [-1.5, 1.0 + 2.0 ** -12, -0.25, 0.0, 1.0, -0.0, 2.0 ** -149, 3.4e38, 1.0 + 2.0 ** -9, -3.4e38, 0.5, 2.0 ** -133,
            -(2.0 ** -149), 2.0 ** -24, 0.0, -0.0]
    dets, gts = [], []
    for j, v in enumerate(vals):
        i = j % 3
        if j % 2 == 0:
            gts.append((i, 1, [8 * j, 0, 4, 4], 0, 0))
        dets.append((i, 1, [8 * j, 0 if j % 2 == 0 else 40, 4, 4], v))
    C["score_values"] = _case(dets, gts, n_img=3, max_dets=[1, 3, 100])
    return C


CASES = _build_cases()
MODULE_CASES = ("area_boundaries", "crowd_rematch", "maxdet_cut_with_ties")

# the sweep: counts of non-ignored ground truths per class
SWEEP_NPIG = list(range(1, 129)) + [200, 250, 255, 256, 257, 300]
SWEEP_PARTIAL = [(5, 3), (20, 13), (50, 49), (7, 0)]  # (ground truths, found): the detections stop early
SWEEP_MAX_DETS = [1, 10, 100000]


def adversarial_rec_thrs():
    """256 ascending recall thresholds (the kernel's limit): 0, 1, every k / n up to n = 16 with its two fp64
    neighbours, the four thresholds of linspace(0, 1, 101) at which ceil(thr * npig) first misses, then k / 17."""
    vals = {0.0, 1.0, float(np.nextafter(0.0, 1.0)), float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0))}
    vals |= {REC_THRS[i] for i in (14, 28, 56, 95)}

    def add(fr):
        v = fr.numerator / fr.denominator
        for x in (float(np.nextafter(v, 0.0)), v, float(np.nextafter(v, 2.0))):
            if len(vals) < 256:
                vals.add(x)

    for n in range(2, 18):
        for k in range(1, n):
            if math.gcd(k, n) == 1:
                add(Fraction(k, n))
    out = sorted(vals)
    assert len(out) == 256 and all(a < b for a, b in zip(out, out[1:]))
    return out


def sweep(rec_thrs, seed=2024):
    """One class per value of SWEEP_NPIG: that many disjoint ground truths, eight per image (each class has images of
    its own), each found by one exact detection at strictly falling scores, with 0..2 unmatched detections before each
    (seeded), so precision is not monotone.  The SWEEP_PARTIAL classes stop finding early: recall < 1."""
    rng = np.random.default_rng(seed)
    dets, gts, img = [], [], 0
    plan = [(n, n) for n in SWEEP_NPIG] + list(SWEEP_PARTIAL)
    for c, (npig, found) in enumerate(plan):
        burst = rng.integers(0, 3, size=npig)
        sc = iter(exact_scores(3 * npig + 3))
        for j in range(npig):
            i, slot = img + j // 8, j % 8
            gts.append((i, c, [4 * slot, 0, 3, 3], 0, 0))
            if j >= found:
                continue
            for f in range(int(burst[j])):
                dets.append((i, c, [4 * slot, 50 + 4 * f, 3, 3], next(sc)))
            dets.append((i, c, [4 * slot, 0, 3, 3], next(sc)))
        img += (npig + 7) // 8
    return _case(dets, gts, n_img=img, iou_thrs=[0.5], rec_thrs=rec_thrs, max_dets=SWEEP_MAX_DETS)


# ---- converters -----------------------------------------------------------------------------------------------------
def cats_of(case):
    return sorted({d[1] for d in case["dets"]} | {g[1] for g in case["gts"]})


def rounded_scores(case, dtype):
    """The case's scores as that type holds them (as fp64 values)."""
    s = torch.tensor([d[3] for d in case["dets"]], dtype=torch.float64)
    return s if dtype == torch.float64 else s.to(dtype).double()


def scores_exact_in(case, dtype):
    s = torch.tensor([d[3] for d in case["dets"]], dtype=torch.float64)
    return torch.equal(rounded_scores(case, dtype), s) and bool((torch.signbit(rounded_scores(case, dtype)) == torch.signbit(s)).all())


def oracle_inputs(case, score_dtype=torch.float64):
    """(dets, gts, cats) as the loop oracle takes them; ground-truth area 0 becomes the box area."""
    sc = rounded_scores(case, score_dtype).tolist()
    dets = [dict(img=i, cat=c, box=b, score=s, area=b[2] * b[3]) for (i, c, b, _), s in zip(case["dets"], sc)]
    gts = [dict(img=i, cat=c, box=b, crowd=cr, area=ar if ar > 0 else b[2] * b[3]) for i, c, b, cr, ar in case["gts"]]
    return dets, gts, cats_of(case)


def run_oracle(case, score_dtype=torch.float64, rules=None):
    """(precision, recall, scores, ious) of the loop oracle as fp64 tensors (ious: the oracle's dict)."""
    dets, gts, cats = oracle_inputs(case, score_dtype)
    p, r, ious, s = coco_oracle.coco_eval(dets, gts, cats, case["n_img"], case["iou_thrs"], case["rec_thrs"],
                                          case["max_dets"], with_scores=True, rules=rules)
    return torch.from_numpy(p), torch.from_numpy(r), torch.from_numpy(s), ious


def flat(case, score_dtype=torch.float64):
    """Flat columns, rows of one image contiguous and in input order; ``gt_area`` with the box-area fallback applied
    (as MeanAveragePrecision hands it to the host and grid evaluators), ``gt_area_raw`` without."""
    d_img = torch.tensor([d[0] for d in case["dets"]], dtype=torch.long)
    g_img = torch.tensor([g[0] for g in case["gts"]], dtype=torch.long)
    do, go = torch.sort(d_img, stable=True)[1], torch.sort(g_img, stable=True)[1]
    det_boxes = torch.tensor([d[2] for d in case["dets"]], dtype=torch.float64).reshape(-1, 4)[do]
    gt_boxes = torch.tensor([g[2] for g in case["gts"]], dtype=torch.float64).reshape(-1, 4)[go]
    raw = torch.tensor([g[4] for g in case["gts"]], dtype=torch.float64)[go]
    scores = torch.tensor([d[3] for d in case["dets"]], dtype=torch.float64)[do]
    cats = torch.tensor(cats_of(case), dtype=torch.long)
    n = case["n_img"]
    offs = lambda img: torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(img, minlength=n).cumsum(0)])  # noqa: E731
    return dict(
        det_boxes=det_boxes, det_scores=scores.to(score_dtype), det_labels=torch.tensor([d[1] for d in case["dets"]], dtype=torch.long)[do],
        det_img=d_img[do], det_area=det_boxes[:, 2] * det_boxes[:, 3], gt_boxes=gt_boxes,
        gt_labels=torch.tensor([g[1] for g in case["gts"]], dtype=torch.long)[go], gt_img=g_img[go],
        gt_crowd=torch.tensor([g[3] for g in case["gts"]], dtype=torch.long)[go], gt_area_raw=raw,
        gt_area=torch.where(raw > 0, raw, gt_boxes[:, 2] * gt_boxes[:, 3]), cats=cats, det_off=offs(d_img), gt_off=offs(g_img),
        n_img=n, iou_thrs=torch.tensor(case["iou_thrs"], dtype=torch.float64), rec_thrs=torch.tensor(case["rec_thrs"], dtype=torch.float64),
        max_dets=torch.tensor(case["max_dets"], dtype=torch.long), area=torch.tensor(coco_oracle.AREA, dtype=torch.float64))


def host_args(x):
    """Arguments of tmx::coco_evaluate (scores as fp64)."""
    return (x["det_boxes"], x["det_scores"].double(), x["det_labels"], x["det_img"], x["det_area"], x["gt_boxes"], x["gt_labels"],
            x["gt_img"], x["gt_crowd"], x["gt_area"], x["cats"], x["n_img"], x["iou_thrs"], x["rec_thrs"], x["max_dets"], x["area"],
            None, None)


def grid_args(x, dev, export_iou=True):
    """Arguments of tmx::coco_evaluate_gpu: class indices by searchsorted, every column on the device."""
    c = lambda t: t.to(dev)  # noqa: E731
    return (c(x["det_boxes"]), c(x["det_scores"]), c(torch.searchsorted(x["cats"], x["det_labels"])), c(x["det_img"]),
            c(x["det_area"]), c(x["gt_boxes"]), c(torch.searchsorted(x["cats"], x["gt_labels"])), c(x["gt_img"]), c(x["gt_crowd"]),
            c(x["gt_area"]), x["cats"].numel(), x["n_img"], c(x["iou_thrs"]), c(x["rec_thrs"]), x["max_dets"], c(x["area"]),
            None, None, None, None, None, export_iou)


def img_args(x, dev, max_dets_dev):
    """Arguments of tmx::coco_evaluate_gpu_img: per-image offsets by bincount().cumsum(), the ground-truth area as
    supplied (the op takes the box area where it is 0)."""
    c = lambda t: t.to(dev)  # noqa: E731
    return (c(x["det_boxes"]), c(x["det_scores"]), c(torch.searchsorted(x["cats"], x["det_labels"])), c(x["det_off"]),
            c(x["gt_boxes"]), c(torch.searchsorted(x["cats"], x["gt_labels"])), c(x["gt_crowd"]), c(x["gt_area_raw"]),
            c(x["gt_off"]), x["cats"].numel(), c(x["iou_thrs"]), c(x["rec_thrs"]), x["max_dets"],
            c(x["max_dets"]) if max_dets_dev else None, c(x["area"]))


def iou_blocks(values, index):
    """{(image, class index): [n_det, n_gt] fp64} of the non-empty blocks of an evaluator's IoU export."""
    values, index = values.cpu(), index.cpu()
    return {(int(r[0]), int(r[1])): values[int(r[4]): int(r[4] + r[2] * r[3])].reshape(int(r[2]), int(r[3]))
            for r in index if r[2] and r[3]}


def oracle_iou_blocks(ious):
    return {key: torch.from_numpy(np.ascontiguousarray(m)) for key, m in ious.items() if m.size}


def module_inputs(case, dev="cpu"):
    """(preds, target) lists of per-image dicts (xywh boxes, fp32 scores) and the MeanAveragePrecision keyword
    arguments that evaluate them with the case's thresholds."""
    preds, target = [], []
    for i in range(case["n_img"]):
        d = [x for x in case["dets"] if x[0] == i]
        g = [x for x in case["gts"] if x[0] == i]
        preds.append(dict(boxes=torch.tensor([x[2] for x in d], dtype=torch.float32, device=dev).reshape(-1, 4),
                          scores=torch.tensor([x[3] for x in d], dtype=torch.float32, device=dev),
                          labels=torch.tensor([x[1] for x in d], dtype=torch.long, device=dev)))
        target.append(dict(boxes=torch.tensor([x[2] for x in g], dtype=torch.float32, device=dev).reshape(-1, 4),
                           labels=torch.tensor([x[1] for x in g], dtype=torch.long, device=dev),
                           iscrowd=torch.tensor([x[3] for x in g], dtype=torch.long, device=dev),
                           area=torch.tensor([x[4] for x in g], dtype=torch.float32, device=dev)))
    kwargs = dict(box_format="xywh", iou_thresholds=case["iou_thrs"], rec_thresholds=case["rec_thrs"],
                  max_detection_thresholds=case["max_dets"])
    return preds, target, kwargs
