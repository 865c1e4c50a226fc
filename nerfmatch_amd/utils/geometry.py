"""Geometry helpers with the reference's call signatures (nerfmatch/utils/geometry.py).

`mutual_nn_matching` (:160-180) is the cosine mutual-nearest-neighbour matcher the NeRF validation step runs on the rendered point
features of a two-view batch.  The reference copies both sets to the host; here device tensors stay on the device and take
nm_feature_mutual_nn (csrc/match_fused.hip, one pass of 128 x 128 similarity tiles that never leaves the registers).  No fallback: a
device tensor without the HIP library raises.  Host tensors take the plain torch statement below, which is the product's behaviour
without a GPU and what the CPU tests compare with the reference's numbers."""
import torch

from .. import ops


def _mutual_nn_torch(desc1, desc2, threshold, eps):
    d1 = desc1 / (desc1.norm(dim=1, keepdim=True) + eps)
    d2 = desc2 / (desc2.norm(dim=1, keepdim=True) + eps)
    sim = d1 @ d2.t()
    s12, nn12 = sim.max(dim=1)
    nn21 = sim.max(dim=0)[1]
    ids1 = torch.arange(sim.shape[0], device=sim.device)
    keep = nn21[nn12] == ids1
    matches, scores = torch.stack([ids1[keep], nn12[keep]], dim=1), s12[keep]
    if threshold:
        keep = scores > threshold
        matches, scores = matches[keep], scores[keep]
    return matches, scores


def mutual_nn_matching(desc1, desc2, threshold=None, eps=1e-9):
    """desc1 (N1, C), desc2 (N2, C) -> matches (K, 2) int64 of (i, j) with j the nearest neighbour of i and i the nearest neighbour of j
    under the cosine similarity of the rows normalised as f / (|f| + eps), in ascending i, and their similarities scores (K,).  A truthy
    `threshold` keeps only scores above it.  An empty side returns the reference's pair of empty (0, 2) int64 tensors."""
    if len(desc1) == 0 or len(desc2) == 0:
        return torch.empty((0, 2), dtype=torch.int64), torch.empty((0, 2), dtype=torch.int64)
    if desc1.is_cuda:
        return ops.feature_mutual_nn(desc1.detach().to(torch.float32).contiguous(), desc2.detach().to(device=desc1.device, dtype=torch.float32).contiguous(),
                                     threshold=threshold, eps=eps)
    return _mutual_nn_torch(desc1, desc2, threshold, eps)
