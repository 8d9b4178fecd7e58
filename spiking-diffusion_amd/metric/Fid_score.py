"""``metric.Fid_score`` surface: main.py's ``from metric.Fid_score import *`` resolves; the distance itself is out of scope."""

__all__ = ["calculate_fid"]


def calculate_fid(images1, images2, use_multiprocessing, batch_size):
    raise NotImplementedError(
        "spkdiff: calculate_fid is outside this build: its activations come from torchvision's "
        "inception_v3(pretrained=True), whose ImageNet weights (inception_v3_google-*.pth) are downloaded from the network. "
        "Reconstruction MSE / SSIM (metric.pytorch_ssim, spkdiff.evaluate) and the operation counts (syops) are implemented.")
