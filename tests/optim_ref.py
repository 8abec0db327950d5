"""NumPy restatements of the four updates of include/nmhip_optim.h, written from TF 1.12's training_ops kernels
(ApplyGradientDescent, ApplyMomentum, ApplyAdagrad, ApplyRMSProp):

    GradientDescent (2)  var -= lr*g
    Momentum (3)         accum = accum*momentum + g;  var -= lr*accum     Nesterov: var -= g*lr + accum*momentum*lr
    Adagrad (4)          accum += g*g;  var -= g*lr*rsqrt(accum)          (no epsilon)
    RMSProp (5)          ms += (g*g - ms)*(1 - decay);  mom = mom*momentum + (g*lr)/sqrt(ms + epsilon);  var -= mom

``g`` is the gradient after the per-tensor clip, applied as oracle/torch_ref.clip_and_adadelta applies it:
g * clip / max(||g||, clip).  ``params`` are the four scalars the kernels take (``Optimizer.params(step)``).  Everything
is evaluated in the dtype of the arrays handed in: float64 for expected values, float32 for the headroom checks."""
import numpy as np

KINDS = (2, 3, 4, 5)
SLOTS = {2: 0, 3: 1, 4: 1, 5: 2}
NAMES = {2: "GradientDescent", 3: "Momentum", 4: "Adagrad", 5: "RMSProp"}


def clip_scale(g, clip):
    """The factor tf.clip_by_norm multiplies ``g`` by (1 when ``clip`` is None or 0)."""
    if not clip:
        return g.dtype.type(1.0)
    dt = g.dtype.type
    norm = np.sqrt((g * g).sum(dtype=g.dtype))
    return dt(clip) / max(norm, dt(clip))


def update(kind, var, g, slot0, slot1, params):
    """One update of one tensor; returns (var, slot0, slot1) as new arrays (a slot the kind lacks comes back as it went
    in, ``None`` included)."""
    dt = var.dtype.type
    p0, p1, p2, p3 = (dt(x) for x in params)
    if kind == 2:
        return var - p0 * g, slot0, slot1
    if kind == 3:
        accum = slot0 * p1 + g
        if p2 != 0:
            return var - (g * p0 + accum * p1 * p0), accum, slot1
        return var - p0 * accum, accum, slot1
    if kind == 4:
        accum = slot0 + g * g
        return var - g * p0 * (dt(1.0) / np.sqrt(accum)), accum, slot1
    if kind == 5:
        ms = slot0 + (g * g - slot0) * (dt(1.0) - p1)
        mom = slot1 * p2 + (g * p0) / np.sqrt(ms + p3)
        return var - mom, ms, mom
    raise ValueError("kind {}".format(kind))


def clip_and_update(kind, p, grads, slot0, slot1, clip, params, names=None):
    """Per-tensor clip then the update of ``kind`` on the tensors ``names`` (default: all of ``p``) of the dicts
    ``p`` / ``slot0`` / ``slot1`` (the slot dicts may be ``None`` where the kind has no such slot), in place.  Returns
    the number of tensors the clip scaled down."""
    clipped = 0
    for k in (list(p) if names is None else names):
        g = np.asarray(grads[k], dtype=p[k].dtype)
        scale = clip_scale(g, clip)
        clipped += int(scale < 1.0)
        a = slot0[k] if slot0 is not None else None
        b = slot1[k] if slot1 is not None else None
        p[k], a, b = update(kind, p[k], g * scale, a, b, params)
        if slot0 is not None:
            slot0[k] = a
        if slot1 is not None:
            slot1[k] = b
    return clipped
