"""``RAFTCriterion``: RAFT's sequence loss and its end-point-error metrics (reference: alonet/raft/criterion.py).

``sequence_loss`` weighs the L1 distance of every iteration's ``up_flow`` to the ground truth by ``gamma ** (T - 1 - t)`` and reports
``loss``, ``epe`` and the 1 / 3 / 5 px inlier rates of the last iteration as Python floats.  Plain torch; the arithmetic is the
reference's, op for op (fixture G21), with one deliberate difference:

  ``valid`` with N > 1.  The reference combines ``valid`` (N, H, W) with the magnitude test (N, 1, H, W) by broadcasting, which for
  N = 1 is the per-pixel mask one expects and for N > 1 is an (N, N, H, W) cross product that then fails with an IndexError when it
  indexes the (N * H * W) end-point errors.  Here ``valid`` is applied per sample — ``valid[n]`` masks sample ``n`` — which is what
  N = 1 does and what the reference evidently intends; for N = 1 the two agree exactly, and N samples at once give the same per-pixel
  terms as N separate N = 1 evaluations (the loss is their mean).
"""
import torch
from torch import nn

import aloscene


class RAFTCriterion(nn.Module):
    def __init__(self):
        super().__init__()

    @staticmethod
    def sequence_loss(m_outputs, flow_gt, valid=None, gamma=0.8, max_flow=400, compute_per_iter=False):
        """``m_outputs``: one dict per iteration with ``up_flow`` (N, 2, H, W); ``flow_gt`` (N, 2, H, W); ``valid`` (N, H, W) or
        ``None``.  Pixels with ``valid < 0.5`` or a ground-truth magnitude of ``max_flow`` or more are excluded (with ``valid=None``
        nothing is, the magnitude test included, as in the reference).  Returns ``(loss, metrics, epe_per_iter)``; ``epe_per_iter``
        is the list of every iteration's end-point errors over the valid pixels, or ``None``."""
        n_predictions = len(m_outputs)
        flow_loss = 0.0

        mag = torch.sum(flow_gt ** 2, dim=1, keepdim=True).sqrt()
        if valid is None:
            valid = torch.ones_like(mag, dtype=torch.bool)
        else:
            valid = (valid[:, None] >= 0.5) & (mag < max_flow)          # (N, 1, H, W): per sample (the module docstring)
        for i in range(n_predictions):
            i_weight = gamma ** (n_predictions - i - 1)
            i_loss = (m_outputs[i]["up_flow"] - flow_gt).abs()
            flow_loss += i_weight * (valid * i_loss).mean()

        def end_point_error(up_flow):
            epe = torch.sum((up_flow - flow_gt) ** 2, dim=1).sqrt()
            return epe.view(-1)[valid.view(-1)]

        epe_per_iter = [end_point_error(m["up_flow"]) for m in m_outputs] if compute_per_iter else None
        epe = end_point_error(m_outputs[-1]["up_flow"])
        metrics = {
            "loss": flow_loss.item(),
            "epe": epe.mean().item(),
            "1px": (epe < 1).float().mean().item(),
            "3px": (epe < 3).float().mean().item(),
            "5px": (epe < 5).float().mean().item(),
        }
        return flow_loss, metrics, epe_per_iter

    def forward(self, m_outputs, frame1, use_valid=True, compute_per_iter=False):
        """``frame1``: the ``aloscene.Frame`` whose ``flow["flow_forward"]`` holds the ground truth, one ``Flow`` per sample.  With
        ``use_valid`` a pixel counts when both ground-truth components are below 1000 in magnitude (RAFT's own rule; the
        occlusion mask is not used)."""
        assert isinstance(frame1, aloscene.Frame)
        flow_gt = [f.batch() for f in frame1.flow["flow_forward"]]
        assert all(f.names == ("B", "C", "H", "W") for f in flow_gt)
        flow_gt = torch.cat([f.as_tensor() for f in flow_gt], dim=0)
        flow_x, flow_y = flow_gt[:, 0, ...], flow_gt[:, 1, ...]
        valid = (flow_x.abs() < 1000) & (flow_y.abs() < 1000) if use_valid else None
        return RAFTCriterion.sequence_loss(m_outputs, flow_gt, valid, compute_per_iter=compute_per_iter)
