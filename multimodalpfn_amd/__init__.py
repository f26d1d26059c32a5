"""MI355X-native drop-in for MultiModalPFN's inference hot path.

``from multimodalpfn_amd import MMPFNClassifier`` replaces
``from mmpfn.models.mmpfn import MMPFNClassifier``, and ``MMPFNRegressor`` likewise; ``ModelInterfaceConfig`` and
``PreprocessorConfig`` live in ``multimodalpfn_amd.constants`` /
``multimodalpfn_amd.preprocessing`` like their reference counterparts.
"""

__all__ = ["MMPFNClassifier", "MMPFNRegressor"]


def __getattr__(name):
    if name == "MMPFNClassifier":
        from multimodalpfn_amd.classifier import MMPFNClassifier

        return MMPFNClassifier
    if name == "MMPFNRegressor":
        from multimodalpfn_amd.regressor import MMPFNRegressor

        return MMPFNRegressor
    raise AttributeError(name)
