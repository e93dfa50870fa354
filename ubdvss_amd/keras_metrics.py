"""Per-batch pixel metrics of the train step -- host mirror of semantic_segmentation/keras_metrics.py:110-191.

The Keras graph evaluates these as extra outputs of every training step; here the fused loss kernel
(csrc/loss.hip) returns the raw counters with the loss (``loss[4:14]``) and the formulas below reproduce the
reference's definitions: accuracy = sum(equal) / max(1, N) (:33-36), precision = tp / max(1, tp + fp) (:66-76),
recall = tp / max(1, tp + fn) (:79-89), f1 = 2PR/(P+R) or 0 (:92-107), classification accuracy over positive
pixels (:160-172), and the loss components of losses.py:138-191.
"""


def metrics_from_loss_vector(loss16, classification_mode=False):
    """loss16: the 16-float vector written by ubd_loss / ubd_train_step (host list / numpy / tensor)."""
    v = [float(x) for x in loss16]
    total, det, cls, _k, pos_l, neg_l, hard_l, n_pos, tp, tn, fp, fn, cls_ok, n_pix = v[:14]
    precision = tp / max(1.0, tp + fp)
    recall = tp / max(1.0, tp + fn)
    out = {
        "loss": total,
        "detection_pixel_acc": (tp + tn) / max(1.0, n_pix),
        "detection_pixel_precision": precision,
        "detection_pixel_recall": recall,
        "detection_pixel_f1": 2.0 * precision * recall / (precision + recall) if precision + recall != 0 else 0.0,
        "positive_loss": pos_l, "negative_loss": neg_l, "hard_negative_loss": hard_l,
    }
    if classification_mode:
        out["classification_pixel_acc"] = cls_ok / max(1.0, n_pos)
        out["detection_loss"] = det
        out["classification_loss"] = cls
    return out


def get_all_metrics(classification_mode=False):
    """Names in the order Keras reports them (keras_metrics.py:175-191)."""
    names = ["detection_pixel_acc", "detection_pixel_precision", "detection_pixel_recall", "detection_pixel_f1"]
    if classification_mode:
        names.append("classification_pixel_acc")
    names += ["positive_loss", "negative_loss", "hard_negative_loss"]
    if classification_mode:
        names += ["detection_loss", "classification_loss"]
    return names


# the order of the device accumulator's value slots (include/ubd.h, ubd_epoch_accumulate): acc[2 + i] is the sum of EPOCH_VALUES[i]
EPOCH_VALUES = ["loss", "detection_pixel_acc", "detection_pixel_precision", "detection_pixel_recall", "detection_pixel_f1",
                "classification_pixel_acc", "positive_loss", "negative_loss", "hard_negative_loss", "detection_loss",
                "classification_loss"]


def epoch_logs_from_sums(acc_host, classification_mode=False, prefix=""):
    """One epoch's logs from the host copy of a ``ubd_epoch_accumulate`` accumulator: ``{prefix + name: sum / seen}`` for ``loss``
    and the names of ``get_all_metrics(classification_mode)``, in that order.  This is Keras 2.2's size-weighted mean of the
    per-batch values -- what ``BaseLogger`` reports for training and ``evaluate_generator`` for ``val_`` -- so the f1 of an epoch
    is the mean of the batches' f1, not the f1 of pooled counters.  ``seen == 0`` (no step was accumulated) raises ValueError:
    there is no mean to report."""
    acc = [float(x) for x in acc_host]
    if len(acc) != 2 + len(EPOCH_VALUES):
        raise ValueError(f"expected {2 + len(EPOCH_VALUES)} accumulator slots, got {len(acc)}")
    seen = acc[0]
    if seen == 0:
        raise ValueError("epoch_logs_from_sums: the accumulator has seen no image")
    sums = dict(zip(EPOCH_VALUES, acc[2:]))
    return {prefix + name: sums[name] / seen for name in ["loss"] + get_all_metrics(classification_mode)}
