"""Float64 host references of the device sampler (sampling.hip) shared by the sampling GPU
tests: the top-k / top-p token set, the order-preserving logit key, and the slot word."""
import numpy as np
import torch


def expected_set(logits, T, k, p):
    """Token set of the host LogitsProcessor (models/sampling.py, candle's
    TopKThenTopP): top-k, then the top-p cutoff on the top-k tokens' FULL-vocabulary
    probabilities (not renormalised: a top-k mass below p keeps all k)."""
    probs = torch.softmax(logits.double() / T, 0)
    keep = torch.ones_like(probs, dtype=torch.bool)
    if k:
        idx = torch.topk(logits, k).indices
        keep = torch.zeros_like(keep)
        keep[idx] = True
    if p is not None and 0 < p < 1:
        pr = torch.where(keep, probs, torch.zeros_like(probs))
        order = torch.argsort(pr, descending=True, stable=True)
        before = torch.cumsum(pr[order], 0) - pr[order]
        kp = torch.zeros_like(keep)
        kp[order[before < p]] = True
        keep &= kp
    return keep


def order_keys(logits):
    """sampling.hip's ordered(): uint32 keys (as int64) whose unsigned order is the float
    order of the f32 logits."""
    u = logits.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)
    u = u.astype(np.int64)
    return np.where(u >> 31 == 0, u ^ 0x80000000, 0xFFFFFFFF - u)


def key_to_float(key):
    """Inverse of ordered() for one uint32 key."""
    key = int(key) & 0xFFFFFFFF
    u = key ^ 0x80000000 if key & 0x80000000 else 0xFFFFFFFF - key
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


def split_slot(slot):
    """int64 slot word(s) -> (value key uint32, token index): the slot holds
    ordered(value) << 32 | ~index."""
    s = np.asarray(slot.detach().cpu().numpy() if isinstance(slot, torch.Tensor) else slot)
    s = s.astype(np.int64).view(np.uint64)
    hi = (s >> np.uint64(32)).astype(np.int64)
    idx = 0xFFFFFFFF - (s & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return hi, idx
