"""Host mirror of the reference's metrics/metric.py and of what evaluate.py reports, computed on the MI355X (kpx_joint_metrics)."""
from .. import ops


def percentual_correct_keypoints(threshold=150):
    """metrics/metric.py:7-16: the share of coordinates with |y_pred - y_true| <= threshold, compared in float32 as TensorFlow does.
    Returns a callable (y_true, y_pred) -> float named percentual_correct_keypoints_<threshold>."""
    def PercentualCorrectKeypoints(y_true, y_pred):
        counts, _, n = ops.joint_metrics(y_true, y_pred, [threshold])
        return float(counts.cpu()[0]) / n if n else float("nan")
    PercentualCorrectKeypoints.__name__ = f"percentual_correct_keypoints_{str(threshold)}"
    return PercentualCorrectKeypoints


def evaluate(model, x, y, thresholds=range(0, 210, 10)):
    """evaluate.py:56-91 on one array of clouds: {"loss": the mean squared error of model.predict(x) against y, "pck": {threshold:
    percentual_correct_keypoints(threshold)}}; one read-back at the end."""
    thresholds = list(thresholds)
    counts, total, n = ops.joint_metrics(y, model.predict(x), thresholds)
    counts, total = counts.cpu().tolist(), float(total.cpu()[0])
    return {"loss": total / n if n else float("nan"), "pck": {t: (c / n if n else float("nan")) for t, c in zip(thresholds, counts)}}
