"""Defense registry (mirror of src/defenses/__init__.py:28-59).

Every name of the reference factory is registered and runs on the HIP kernels
(FLTrust's server update runs on the client-batched trainer).
"""
from .base_defense import BaseDefense, CenteredDefense, NoDefense
from .bulyan import BulyanDefense
from .centered_clipping import CenteredClippingDefense
from .dnc import DnCDefense
from .krum import KrumDefense, KrumTrimmedMeanDefense, MultiKrumDefense
from .flame import FlameDefense
from .fltrust import FLTrustDefense
from .foolsgold import FoolsGoldDefense
from .geometric_median import GeometricMedianDefense
from .norm_based import DPSGDDefense, GradientClippingDefense, NormBoundingDefense
from .robust_lr import RobustLRDefense
from .sparsefed import SparseFedDefense
from .trimmed_mean import MedianDefense, TrimmedMeanDefense

__all__ = [
    "BaseDefense", "CenteredDefense", "NoDefense", "KrumDefense", "MultiKrumDefense", "KrumTrimmedMeanDefense", "BulyanDefense",
    "TrimmedMeanDefense", "MedianDefense", "GeometricMedianDefense",
    "GradientClippingDefense", "NormBoundingDefense", "DPSGDDefense", "FLTrustDefense", "CenteredClippingDefense",
    "DnCDefense", "FoolsGoldDefense", "RobustLRDefense", "FlameDefense", "SparseFedDefense",
    "get_defense", "defense_names",
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

# The names added since tests/test_defense_layer_host.py fixed _DEFENSES' key set and each entry's engine
# flags (its test_engine_table); a name here has those flags checked by its own tests.
_LATER_DEFENSES = {
    # FLAME (USENIX Security 2022): the majority cluster of the cosine distances, median clipping, Gaussian noise
    "flame": FlameDefense,
    # SparseFed (AISTATS 2022): clipped mean into a server-side error memory, only its top-k coordinates applied
    "sparsefed": SparseFedDefense,
}


def defense_names():
    """Every name get_defense takes."""
    return list(_DEFENSES) + list(_LATER_DEFENSES)


def get_defense(defense_type: str, defense_config: dict):
    """Factory by name; unknown names raise ValueError like the reference."""
    cls = _DEFENSES.get(defense_type) or _LATER_DEFENSES.get(defense_type)
    if cls is None:
        raise ValueError(f"Unknown defense type: {defense_type}. Available: {defense_names()}")
    return cls(defense_config)
