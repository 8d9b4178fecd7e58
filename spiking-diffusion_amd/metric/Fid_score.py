"""``metric.Fid_score`` surface: main.py's ``from metric.Fid_score import *`` resolves.  The Inception activations are out of
scope (``calculate_fid`` raises); the distance between two Gaussian fits is here, in the reference's own convention."""

__all__ = ["calculate_fid", "calculate_frechet_distance"]


def calculate_fid(images1, images2, use_multiprocessing, batch_size):
    raise NotImplementedError(
        "spkdiff: calculate_fid is outside this build: its activations come from torchvision's "
        "inception_v3(pretrained=True), whose ImageNet weights (inception_v3_google-*.pth) are downloaded from the network. "
        "Reconstruction MSE / SSIM (metric.pytorch_ssim, spkdiff.evaluate) and the operation counts (syops) are implemented.")


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """R/metric/Fid_score.py:116-172 by name, signature and convention: |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr(U sqrt(S) V)
    with U S V the SVD of sigma1 sigma2 -- the Frechet distance only where the covariances commute;
    ``spkdiff.evaluate.frechet_distance(..., 'exact')`` is the distance itself.  ``eps`` is the reference's regulariser for a
    non-finite square root, which an SVD of finite matrices never produces: it is accepted and not read."""
    from spkdiff.evaluate import frechet_distance
    return frechet_distance((mu1, sigma1), (mu2, sigma2), "reference")
