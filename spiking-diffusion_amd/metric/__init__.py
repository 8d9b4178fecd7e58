"""Drop-in ``metric`` package of the MI355X build (the module names of R/metric): ``pytorch_ssim`` is implemented,
``IS_score`` and ``Fid_score`` keep their entry points and raise (they need Inception weights from the network)."""
