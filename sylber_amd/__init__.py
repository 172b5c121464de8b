"""sylber_amd — MI355X-native implementation of the SYLBER ``Segmenter`` forward path
(reference API: sylber/__init__.py:1 exports ``Segmenter``) and of ``SegmentSynthesis.resynthesize``."""
from .segmenter import Segmenter, HubertEncoderHIP  # noqa: F401
from .synthesis import SegmentSynthesis  # noqa: F401
from .downstream import (KMQuantizer, ResidualKMQuantizer, expand_feature, load_km_quantizer,  # noqa: F401
                         load_residualkm_quantizer)
from .quantizer import Quantizer, load_quantizer  # noqa: F401
from .kmeans import KMeansFit, fit_kmeans, fit_km_quantizer, fit_residual_km_quantizer  # noqa: F401
from .search import IVFSyllableIndex, SyllableIndex, align_sequences, local_align_sequences  # noqa: F401
from .pq import IVFPQSyllableIndex, PQSyllableIndex  # noqa: F401
from .units import UnitErrorRate, UnitIndex, align_unit_strings, local_align_unit_strings, local_align_unit_strings_all, unit_error_rate  # noqa: F401

__all__ = ["Segmenter", "HubertEncoderHIP", "SegmentSynthesis", "KMQuantizer", "ResidualKMQuantizer", "expand_feature",
           "load_km_quantizer", "load_residualkm_quantizer", "Quantizer", "load_quantizer",
           "KMeansFit", "fit_kmeans", "fit_km_quantizer", "fit_residual_km_quantizer", "SyllableIndex", "IVFSyllableIndex",
           "PQSyllableIndex", "IVFPQSyllableIndex", "UnitIndex", "UnitErrorRate", "align_unit_strings", "unit_error_rate",
           "local_align_unit_strings", "local_align_unit_strings_all", "align_sequences", "local_align_sequences"]
