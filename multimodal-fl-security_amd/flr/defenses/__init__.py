"""Defense registry (mirror of src/defenses/__init__.py:28-59).

Every name of the reference factory is registered and runs on the HIP kernels
(FLTrust's server update runs on the client-batched trainer).
"""
from .base_defense import BaseDefense, CenteredDefense, NoDefense
from .bulyan import BulyanDefense
from .centered_clipping import CenteredClippingDefense
from .dnc import DnCDefense
from .krum import KrumDefense, KrumTrimmedMeanDefense, MultiKrumDefense
from .fltrust import FLTrustDefense
from .foolsgold import FoolsGoldDefense
from .geometric_median import GeometricMedianDefense
from .norm_based import DPSGDDefense, GradientClippingDefense, NormBoundingDefense
from .robust_lr import RobustLRDefense
from .trimmed_mean import MedianDefense, TrimmedMeanDefense

__all__ = [
    "BaseDefense", "CenteredDefense", "NoDefense", "KrumDefense", "MultiKrumDefense", "KrumTrimmedMeanDefense", "BulyanDefense",
    "TrimmedMeanDefense", "MedianDefense", "GeometricMedianDefense",
    "GradientClippingDefense", "NormBoundingDefense", "DPSGDDefense", "FLTrustDefense", "CenteredClippingDefense",
    "DnCDefense", "FoolsGoldDefense", "RobustLRDefense",
    "get_defense",
]

_DEFENSES = {
    "none": NoDefense,
    "fedavg": NoDefense,
    "krum": KrumDefense,
    "multi_krum": MultiKrumDefense,
    "trimmed_mean": TrimmedMeanDefense,
    "median": MedianDefense,
    "geometric_median": GeometricMedianDefense,
    "dp_sgd": DPSGDDefense,
    "gradient_clipping": GradientClippingDefense,
    "norm_bounding": NormBoundingDefense,
    "fltrust": FLTrustDefense,
    # build extension: Multi-Krum selection then trimmed mean (BASELINE.json configs[4])
    "krum_trimmed_mean": KrumTrimmedMeanDefense,
    # Bulyan (ICML 2018): iterated Krum selection, then the median-window mean
    "bulyan": BulyanDefense,
    # centered clipping (ICML 2021): iterated clipped mean around the previous global model
    "centered_clipping": CenteredClippingDefense,
    # divide-and-conquer (NDSS 2021): spectral filtering on subsampled coordinates, then the kept rows' mean
    "dnc": DnCDefense,
    # FoolsGold (RAID 2020): sybils resemble each other; weights from the clients' pairwise cosine similarity
    "foolsgold": FoolsGoldDefense,
    # robust learning rate (AAAI 2021): a per-coordinate sign vote negates the step where too few clients agree
    "robust_lr": RobustLRDefense,
}


def get_defense(defense_type: str, defense_config: dict):
    """Factory by name; unknown names raise ValueError like the reference."""
    if defense_type not in _DEFENSES:
        raise ValueError(f"Unknown defense type: {defense_type}. Available: {list(_DEFENSES.keys())}")
    return _DEFENSES[defense_type](defense_config)
