"""Host-side mirror of ``bm/losses.py``'s ``ClipLoss`` (the contrastive head of the hot path):
same constructor, ``forward`` / ``get_scores`` / ``get_probabilities`` / ``trim_samples`` with the
reference's argument meaning and assertion behaviour; the contraction over K = F*T, the candidate
norms, the row softmax / cross-entropy and the backward GEMM are libbmhip kernels.
"""
import typing as tp

import torch

from . import functional as BF


class ClipLoss(torch.nn.Module):
    """CLIP contrastive loss (bm/losses.py:29-114).

    ``linear`` is accepted and, exactly like in the reference, never applied: the reference sets
    ``self.linear = None`` (losses.py:35) and only tests that attribute (losses.py:82)."""

    def __init__(self, linear=None, twin=True, pool=False, tmin=None, tmax=None,
                 tmin_train=None, tmax_train=None, dset_args=None, center=False, symmetric=False):
        super().__init__()
        # extension (default off = the reference): add the column term of the CLIP objective, loss =
        # (CE over each estimate's row + CE over each target candidate's column) / 2
        self.symmetric = symmetric
        self.linear = None
        self.pool = pool
        self.center = center
        if linear is not None:
            self.linear_est = torch.nn.LazyLinear(linear)
            self.linear_gt = self.linear_est if twin else torch.nn.LazyLinear(linear)
        self.tmin = tmin
        self.tmax = tmax
        self.tmin_train = tmin_train
        self.tmax_train = tmax_train
        self.dset_args = dset_args
        self.defer_mask_check = False       # brainmagick_amd.solver.Solver sets it (see forward)

    def trim_samples(self, estimates, candidates):
        """Crop both [B, C, T] tensors to the samples between (tmin, tmax) seconds, counted from
        ``dset_args.tmin`` at ``dset_args.sample_rate`` (losses.py:50-75)."""
        use_train = self.training and (self.tmin_train is not None or self.tmax_train is not None)
        tmin, tmax = (self.tmin_train, self.tmax_train) if use_train else (self.tmin, self.tmax)
        lo, hi = 0, estimates.shape[-1]
        if tmin is not None or tmax is not None:
            assert self.dset_args is not None
            assert self.dset_args.tmin is not None
            origin, rate = self.dset_args.tmin, self.dset_args.sample_rate
            if tmin is not None:
                assert tmin >= origin, 'clip.tmin should be above dset.tmin'
                lo = int((-origin + tmin) * rate)
            if tmax is not None:
                hi = int((-origin + tmax) * rate)
        if lo == 0 and hi == estimates.shape[-1] and hi == candidates.shape[-1]:
            # no crop: the tensors themselves go on (a slice would be a new object without the maxima / candidate
            # norms their producers published)
            return estimates, candidates
        return estimates[..., lo:hi], candidates[..., lo:hi]

    def _prepare(self, estimates, candidates):
        estimates, candidates = self.trim_samples(estimates, candidates)
        # pool / center are off in every configuration of the paper (conf/config.yaml:56-64); they
        # are cheap pre-reductions done with torch ops on the GPU before the HIP contraction.
        if self.pool:
            estimates = estimates.mean(dim=2, keepdim=True)
            candidates = candidates.mean(dim=2, keepdim=True)
        if self.center:
            estimates = estimates - estimates.mean(dim=(1, 2), keepdim=True)
            candidates = candidates - candidates.mean(dim=(1, 2), keepdim=True)
        if not estimates.is_cuda:
            raise RuntimeError("brainmagick_amd.ClipLoss runs on the MI355X HIP path only "
                               "(no CPU fallback)")
        return estimates.contiguous(), candidates.contiguous()

    def get_scores(self, estimates: torch.Tensor, candidates: torch.Tensor):
        """[B, C, T] x [B', C, T] -> [B, B'] matching scores (losses.py:77-95)."""
        estimates, candidates = self._prepare(estimates, candidates)
        if torch.is_grad_enabled() and estimates.requires_grad:
            return BF.ClipLossFn.apply(estimates, candidates)[1]
        return BF.clip_scores(estimates, candidates)

    def get_probabilities(self, estimates, candidates):
        """[B, B'] row-softmax of the scores (losses.py:97-102)."""
        estimates, candidates = self._prepare(estimates, candidates)
        return BF.clip_scores(estimates.detach(), candidates.detach(), want_probs=True)

    def forward(self, estimate, candidate, mask=None, target_offset: int = 0, candidate_valid=None, estimate_all=None):
        """The first B candidates are the targets of the B estimates, the remaining B'-B are only
        negatives (losses.py:104-114).  ``target_offset`` (extension, default 0 = reference
        behaviour) shifts the targets to candidates [offset, offset+B): a data-parallel rank uses
        it to point at its own block of the whole-node gathered candidates.  ``candidate_valid``
        (extension, [B'] fp32, default None = all): candidates marked 0 are padding (ranks that rejected
        different numbers of segments bring equal-sized, partly empty blocks) and never count as negatives.
        ``estimate_all`` (extension, with ``symmetric``): the estimates of EVERY rank, gathered with an autograd-aware
        all-gather, this rank's block at rows [offset, offset+B) -- the column term then lets each of this rank's target
        candidates classify the whole node's estimates (north_star: "all-gather of brain/audio embeddings ... so the
        negatives pool is whole-node" for the column softmax too); without it the column term sees the local estimates."""
        if self.defer_mask_check and mask.is_cuda and mask.dtype == torch.bool:
            # Solver: the reference's assert costs a host sync in the middle of the step; the verdict is OR-ed into
            # the device-side flag word and raised at the next step's single synchronisation point
            from . import hip_ops as H
            H.flag_unless_all_set(mask if mask.is_contiguous() else mask.contiguous(),
                                  H.index_error_flag(mask.device)[2:3])
        else:
            assert mask.all(), "mask is not supported for now"
        assert estimate.size(0) + target_offset <= candidate.size(0), \
            "need at least as many targets as estimates"
        if self.symmetric and estimate_all is not None:
            return self._symmetric_over_the_node(estimate, candidate, target_offset, candidate_valid, estimate_all)
        estimate, candidate = self._prepare(estimate, candidate)
        return BF.ClipLossFn.apply(estimate, candidate, target_offset, candidate_valid, self.symmetric)[0]

    def _symmetric_over_the_node(self, estimate, candidate, target_offset, candidate_valid, estimate_all):
        """(row term + column term) / 2 with whole-node negatives on BOTH sides.  Row term: this rank's estimates
        against all candidates (as without ``symmetric``).  Column term: this rank's target candidates j against ALL
        estimates i, CE over i of s[i, j] = est_i . cand_j / ||cand_j|| with the target at row offset + j -- computed as
        the row term of the transposed problem: "estimates" = the target candidates scaled by their inverse norms,
        "candidates" = the gathered estimates, unnormalised; its gradient flows into ``estimate_all`` and through the
        all-gather's adjoint (a reduce-scatter) back to every rank's encoder."""
        if candidate_valid is not None:
            raise NotImplementedError("the node-wide column term needs the same number of segments on every rank "
                                      "(candidate_valid marks padding blocks of ranks that rejected segments)")
        if candidate.requires_grad:
            raise NotImplementedError("the node-wide column term is built for constant candidates")
        from . import hip_ops as H
        B = estimate.size(0)
        assert estimate_all.size(0) >= target_offset + B
        est, cand = self._prepare(estimate, candidate)
        rows = BF.ClipLossFn.apply(est, cand, target_offset, None, False)[0]
        est_all, _ = self._prepare(estimate_all, candidate)
        targets = cand[target_offset:target_offset + B]
        inv = H.clip_inv_norms(targets.contiguous())
        scaled = (targets * inv.view(-1, 1, 1)).contiguous()
        cols = BF.ClipLossFn.apply(scaled, est_all, target_offset, None, False, False)[0]
        return 0.5 * (rows + cols)


class _MaskedLoss(torch.nn.Module):
    """bm/losses.py:11-14: the loss over ``estimate[mask.expand_as(estimate)]`` -- here without the gather: the kernels
    read the mask in place ([B, 1, T] or [B, F, T] bool).  ``mask=None`` means all true (an extension: the reference
    would fail on None)."""
    kind = ""

    def __init__(self):
        super().__init__()
        self.no_mask_flag = None    # Solver: int32 device word that receives the "no mask!" bit (bm/solver.py:354-356)

    def forward(self, estimate, output, mask=None):
        if not (estimate.is_cuda and output.is_cuda):
            raise RuntimeError(f"brainmagick_amd.{type(self).__name__} runs on the MI355X HIP path only "
                               "(no CPU fallback)")
        if mask is not None:
            if mask.dtype != torch.bool:
                raise TypeError(f"mask must be a bool tensor (the reference indexes with it), got {mask.dtype}")
            mask.expand_as(estimate)       # the reference's shape rule: broadcastable to the estimate
        return BF.MaskedRegressionFn.apply(estimate, output, mask, self.kind, self.no_mask_flag)[0]


class L1Loss(_MaskedLoss):
    """torch.nn.L1Loss() over the selected elements (bm/losses.py:17-20)."""
    kind = "l1"


class L2Loss(_MaskedLoss):
    """torch.nn.MSELoss() over the selected elements (bm/losses.py:23-26)."""
    kind = "mse"


class FeatureDecodingLoss(torch.nn.Module):
    """bm/losses.py:117-173 (`optim.loss: regression_classification`): MSE on the continuous features of
    ``used_features`` plus cross-entropy on the categorical ones, every term a mean over the positions ``mask`` selects,
    summed in feature order -- one forward and one backward kernel launch for the whole loss (csrc/regress.hip), no
    gather, no transpose, no read-back.

    ``used_features`` is what the reference hands over (bm.features.FeaturesBuilder), duck-typed: ``.values()``,
    ``.get_slice(name, model_output=...)``, ``.dimension``, ``.output_dimension``; every feature has ``.name``,
    ``.categorical``, ``.dimension``, ``.output_dimension``.  ``scaler``: None (unweighted; `optim.use_weighting` off),
    a ``norm.DeviceBatchScaler`` or anything else with ``get_categorical_feature_weights(name)``; the class weights are
    fetched once and kept on the device in one vector.

    ``mask``: bool [B, 1, T] (the only shape the reference's categorical branch can index with) or None = all true (an
    extension, as for L1Loss / L2Loss).  A class is the target channel truncated towards zero (``.long()``); -100
    (torch's ignore_index) has NO special meaning here -- the reference's features never produce it -- and is out of
    range like any other negative class.  The reference's two synchronising asserts (``mask.any()``, losses.py:133, and
    "categories up to", losses.py:150) become bits of ``no_mask_flag`` (an int32 device word, set by the Solver): a
    position with an out-of-range class contributes nothing, an empty mask gives NaN.  ``last_terms``: the per-feature
    terms of the last call, a device tensor (no sync).  The gradient goes to the estimate only."""

    def __init__(self, used_features, scaler):
        super().__init__()
        self.used_features = used_features
        self.scaler = scaler
        self.no_mask_flag = None    # Solver: the flag word slot that receives NO_MASK_BIT / CATEGORY_RANGE_BIT
        self.last_terms: tp.Optional[torch.Tensor] = None
        self._table = None
        self._weights: tp.Dict[torch.device, tp.Optional[torch.Tensor]] = {}

    def _plan(self):
        """((kind, est_start, width, out_start, weight_off) per feature, host weights | None), built once."""
        if self._table is None:
            from . import hip_ops as H
            rows, weights, n_weights = [], [], 0
            for feature in self.used_features.values():
                name = feature.name
                sl = self.used_features.get_slice(name)
                sl_out = self.used_features.get_slice(name, model_output=True)
                if feature.categorical:
                    assert sl.stop - sl.start == 1, \
                        "Supporting only single categorical cross entropy for now."
                    off = -1
                    if self.scaler:
                        w = self.scaler.get_categorical_feature_weights(name).detach().float().cpu().flatten()
                        if w.numel() != sl_out.stop - sl_out.start:
                            raise ValueError(f"feature {name}: {w.numel()} class weights for "
                                             f"{sl_out.stop - sl_out.start} classes")
                        off = n_weights
                        weights.append(w)
                        n_weights += w.numel()
                    rows.append((H.FEATURE_CATEGORICAL, sl_out.start, sl_out.stop - sl_out.start, sl.start, off))
                else:
                    assert sl_out.stop - sl_out.start == sl.stop - sl.start, name
                    rows.append((H.FEATURE_CONTINUOUS, sl_out.start, sl.stop - sl.start, sl.start, -1))
            self._table = tuple(rows), (torch.cat(weights) if weights else None)
        return self._table

    def forward(self, estimate, output, mask=None):
        assert estimate.shape[1] == self.used_features.output_dimension and \
               output.shape[1] == self.used_features.dimension, \
               "Invalid features dim received. Are you using the correct " \
               "features for the loss?"
        if mask is not None:
            if mask.dtype != torch.bool:
                raise TypeError(f"mask must be a bool tensor (the reference indexes with it), got {mask.dtype}")
            if tuple(mask.shape) != (estimate.shape[0], 1, estimate.shape[-1]):
                raise ValueError(f"mask must be [B, 1, T] = {(estimate.shape[0], 1, estimate.shape[-1])} (what the "
                                 f"reference's categorical branch can index with), got {tuple(mask.shape)}")
        if output.requires_grad:
            raise NotImplementedError("FeatureDecodingLoss sends no gradient to the targets (a learnable feature model "
                                      "is not supported with it)")
        if not (estimate.is_cuda and output.is_cuda):
            raise RuntimeError("brainmagick_amd.FeatureDecodingLoss runs on the MI355X HIP path only (no CPU fallback)")
        table, host_weights = self._plan()
        if estimate.device not in self._weights:
            self._weights[estimate.device] = None if host_weights is None else host_weights.to(estimate.device)
        loss, terms, _ = BF.FeatureDecodingFn.apply(estimate, output, mask, table, self._weights[estimate.device],
                                                    self.no_mask_flag)
        self.last_terms = terms
        return loss


def create_loss(name: str, used_features=None, scaler=None, **clip_kw) -> torch.nn.Module:
    """The loss factory of bm/solver.py:76-94 (`optim.loss`): 'l1', 'mse', 'clip' (``clip_kw`` = the `clip:`
    configuration block, plus ``dset_args``) or 'regression_classification' (``used_features`` = the features builder,
    ``scaler`` = the fitted scaler when `optim.use_weighting`, else None)."""
    if name == "l1":
        return L1Loss()
    if name == "mse":
        return L2Loss()
    if name == "clip":
        kw = dict(clip_kw)
        kw.pop("save_best", None)
        kw.pop("sync_grad", None)
        return ClipLoss(**kw)
    if name == "regression_classification":
        if used_features is None:
            raise NotImplementedError("optim.loss='regression_classification' (FeatureDecodingLoss) needs the features "
                                      "builder: create_loss(name, used_features=..., scaler=...)")
        return FeatureDecodingLoss(used_features, scaler)
    raise ValueError(f"Unsupported loss {name}")
