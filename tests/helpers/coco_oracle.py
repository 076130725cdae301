"""Straight-line Python statement of the COCO evaluate / accumulate / summarize algorithm (per-image,
per-category greedy matching, envelope precision, recall-threshold sampling).  Used as an independent oracle
for the native evaluator; deliberately written loop-by-loop without any vectorisation.

Every rule of pycocotools' ``evaluateImg`` / ``accumulate`` that a matcher can get wrong is one small method of
``Oracle``, so a test can state a wrong reading of one rule in one line (a subclass overriding that method) and
check that its cases tell the two apart; ``coco_eval`` runs the rules as published."""
import numpy as np

AREA = [[0, 1e10], [0, 32**2], [32**2, 96**2], [96**2, 1e10]]


def _iou(d, g, crowd):
    out = np.zeros((len(d), len(g)))
    for i, a in enumerate(d):
        for j, b in enumerate(g):
            w = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
            h = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
            if w <= 0 or h <= 0:
                continue
            inter = w * h
            u = a[2] * a[3] if crowd[j] else a[2] * a[3] + b[2] * b[3] - inter
            out[i, j] = inter / u
    return out


class Oracle:
    """pycocotools' rules, one per method (evaluateImg: cocoeval.py:236-313, accumulate: :315-420)."""

    # ---- evaluateImg
    def det_order(self, scores):  # np.argsort(-scores, kind="mergesort"): python's sort is stable too
        return sorted(range(len(scores)), key=lambda j: -scores[j])

    def gt_outside(self, area, lo, hi):  # g["area"] < aRng[0] or g["area"] > aRng[1]
        return area < lo or area > hi

    def det_outside(self, area, lo, hi):  # an unmatched detection outside the range is ignored
        return area < lo or area > hi

    def taken(self, matched, crowd):  # if gtm[tind, gind] > 0 and not iscrowd[gind]: continue
        return matched > 0 and not crowd

    def stop_at_ignored(self, m, gig, gi):  # if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1: break
        return m > -1 and gig[m] == 0 and gig[gi] == 1

    def below(self, iou, best, m):  # if ious[dind, gind] < iou: continue   (m: the match so far, -1 for none)
        return iou < best

    # ---- accumulate
    def merge_order(self, sc):  # inds = np.argsort(-dtScores, kind="mergesort") over the images in image order
        return np.argsort(-sc, kind="mergesort")

    def envelope(self, pr):  # for i in range(nd - 1, 0, -1): if pr[i] > pr[i - 1]: pr[i - 1] = pr[i]
        for j in range(len(pr) - 1, 0, -1):
            if pr[j] > pr[j - 1]:
                pr[j - 1] = pr[j]

    def recall_index(self, rc, tp, npig, rec_thrs):  # inds = np.searchsorted(rc, p.recThrs, side="left")
        return np.searchsorted(rc, rec_thrs, side="left")

    def answer(self, thr, value):  # q[ri] = pr[pi]; ss[ri] = dtScoresSorted[pi]
        return value

    # ---- the algorithm
    def evaluate(self, dets, gts, cats, n_img, iou_thrs, max_dets, iou_fn=None, area=None):
        area = AREA if area is None else area
        T = len(iou_thrs)
        d_of, g_of = {}, {}  # (image, class) -> rows in input order, built once
        for x in dets:
            d_of.setdefault((x["img"], x["cat"]), []).append(x)
        for x in gts:
            g_of.setdefault((x["img"], x["cat"]), []).append(x)
        evals = {}
        ious = {}
        for i in range(n_img):
            for k, c in enumerate(cats):
                d = d_of.get((i, c), [])
                g = g_of.get((i, c), [])
                order = self.det_order([x["score"] for x in d])
                d = [d[j] for j in order][: max_dets[-1]]
                if iou_fn is None:
                    ious[(i, k)] = _iou([x["box"] for x in d], [x["box"] for x in g], [x["crowd"] for x in g])
                else:
                    ious[(i, k)] = iou_fn(d, g)
                for a, (lo, hi) in enumerate(area):
                    if not d and not g:
                        evals[(k, a, i)] = None
                        continue
                    gig = [1 if (x["crowd"] or self.gt_outside(x["area"], lo, hi)) else 0 for x in g]
                    gorder = sorted(range(len(g)), key=lambda j: gig[j])
                    gs = [g[j] for j in gorder]
                    gig = [gig[j] for j in gorder]
                    crowd = [x["crowd"] for x in gs]
                    io = ious[(i, k)][:, gorder] if len(d) and len(g) else np.zeros((len(d), len(g)))
                    gtm = np.zeros((T, len(g)))
                    dtm = np.zeros((T, len(d)))
                    dig = np.zeros((T, len(d)))
                    for t, thr in enumerate(iou_thrs):
                        for di in range(len(d)):
                            best = min(thr, 1 - 1e-10)
                            m = -1
                            for gi in range(len(g)):
                                if self.taken(gtm[t, gi], crowd[gi]):
                                    continue
                                if self.stop_at_ignored(m, gig, gi):
                                    break
                                if self.below(io[di, gi], best, m):
                                    continue
                                best = io[di, gi]
                                m = gi
                            if m == -1:
                                continue
                            dig[t, di] = gig[m]
                            dtm[t, di] = 1
                            gtm[t, m] = 1
                    for di, x in enumerate(d):
                        if self.det_outside(x["area"], lo, hi):
                            for t in range(T):
                                if dtm[t, di] == 0:
                                    dig[t, di] = 1
                    evals[(k, a, i)] = dict(scores=[x["score"] for x in d], dtm=dtm, dig=dig, gig=np.array(gig))
        return evals, ious

    def accumulate(self, evals, K, n_img, T, rec_thrs, max_dets, A=len(AREA)):
        R, M = len(rec_thrs), len(max_dets)
        rec_thrs = np.asarray(rec_thrs, dtype=np.float64)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        for k in range(K):
            for a in range(A):
                for m, md in enumerate(max_dets):
                    E = [evals[(k, a, i)] for i in range(n_img) if evals[(k, a, i)] is not None]
                    if not E:
                        continue
                    sc = np.concatenate([np.array(e["scores"][:md], dtype=np.float64) for e in E])
                    inds = self.merge_order(sc)
                    sc_sorted = sc[inds]
                    dtm = np.concatenate([e["dtm"][:, :md] for e in E], axis=1)[:, inds]
                    dig = np.concatenate([e["dig"][:, :md] for e in E], axis=1)[:, inds]
                    gig = np.concatenate([e["gig"] for e in E])
                    npig = np.count_nonzero(gig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dig))
                    tp_sum = np.cumsum(tps, axis=1).astype(float)
                    fp_sum = np.cumsum(fps, axis=1).astype(float)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        nd = len(tp)
                        rc = tp / npig
                        pr = (tp / (fp + tp + np.spacing(1))).tolist()
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        self.envelope(pr)
                        q = np.zeros(R)
                        ss = np.zeros(R)
                        idx = self.recall_index(rc, tp, npig, rec_thrs)
                        for ri, pi in enumerate(idx):
                            if pi >= nd:
                                break
                            q[ri] = self.answer(rec_thrs[ri], pr[pi])
                            ss[ri] = self.answer(rec_thrs[ri], sc_sorted[pi])
                        precision[t, :, k, a, m] = q
                        scores[t, :, k, a, m] = ss
        return precision, recall, scores


def coco_eval(dets, gts, cats, n_img, iou_thrs, rec_thrs, max_dets, iou_fn=None, area=None, with_scores=False,
              rules=None):
    """dets: list of dicts(img, cat, box(xywh), score, area); gts: list of dicts(img, cat, box, crowd, area).

    Returns (precision [T, R, K, A, M], recall [T, K, A, M], ious {(image, class index): [n_det, n_gt]}), and with
    ``with_scores`` a fourth result: pycocotools' score table [T, R, K, A, M] (the sorted score at the searchsorted
    index; 0 where the precision is 0 by lack of recall).  ``area`` replaces the module constant ``AREA``."""
    rules = Oracle() if rules is None else rules
    evals, ious = rules.evaluate(dets, gts, cats, n_img, iou_thrs, max_dets, iou_fn, area)
    A = len(AREA if area is None else area)
    precision, recall, scores = rules.accumulate(evals, len(cats), n_img, len(iou_thrs), rec_thrs, max_dets, A)
    if with_scores:
        return precision, recall, ious, scores
    return precision, recall, ious


def summarize(precision, recall, iou_thrs, max_dets, first_max_det=100):
    def s(ap, thr=None, area=0, md=100):
        mind = [i for i, v in enumerate(max_dets) if v == md]
        x = precision[..., area, mind] if ap else recall[..., area, mind]
        if thr is not None:
            x = x[[i for i, v in enumerate(iou_thrs) if v == thr]]
        v = x[x > -1]
        return -1.0 if v.size == 0 else float(np.mean(v))

    m2 = max_dets[2]
    return [
        s(1, md=first_max_det), s(1, 0.5, md=m2), s(1, 0.75, md=m2), s(1, area=1, md=m2), s(1, area=2, md=m2),
        s(1, area=3, md=m2), s(0, md=max_dets[0]), s(0, md=max_dets[1]), s(0, md=m2), s(0, area=1, md=m2),
        s(0, area=2, md=m2), s(0, area=3, md=m2),
    ]
