"""``metric.IS_score`` surface: main.py's ``from metric.IS_score import *`` resolves; the score itself is out of scope."""

__all__ = ["inception_score"]


def inception_score(imgs, cuda=True, batch_size=32, resize=False, splits=1):
    raise NotImplementedError(
        "spkdiff: inception_score is outside this build: it classifies the samples with torchvision's "
        "inception_v3(pretrained=True), whose ImageNet weights (inception_v3_google-*.pth) are downloaded from the network. "
        "Reconstruction MSE / SSIM (metric.pytorch_ssim, spkdiff.evaluate) and the operation counts (syops) are implemented.")
