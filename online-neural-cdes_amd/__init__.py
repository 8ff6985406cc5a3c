"""MI355X-native Neural-CDE forward/adjoint integrator: a drop-in for the reference's
``torchcde.cdeint`` / ``src.ncde.NeuralCDE`` hot path.  Import as ``ncde_amd`` (see ncde_amd.py).

The compute path is hand-written HIP for gfx950 behind a C-ABI (include/ncde_hip.h); this package is
the thin Python host mirroring the reference's call surface.  There is no CPU fallback.
"""
from . import data  # noqa: F401
from ._lib import NcdeError, lib  # noqa: F401
from .interpolation import CubicSpline, LinearInterpolation, NaturalCubicSpline, SmoothLinearInterpolation  # noqa: F401
from .solver import FieldSpec, cdeint, coop_status  # noqa: F401
from .vector_fields import (GRUGatedVectorField, LowRankVectorField, MinimalGatedVectorField, MLPField,  # noqa: F401
                            OriginalVectorField)
from .ncde import NeuralCDE  # noqa: F401
from .online import OnlineNeuralCDE, OnlineStackedNeuralCDE  # noqa: F401
from .stacked import StackedNeuralCDE  # noqa: F401
from .coefficients import (forward_fill, hermite_cubic_coefficients_with_backward_differences, linear_interpolation_coeffs,  # noqa: F401
                           linear_rectilinear_hybrid_coeffs, natural_cubic_coeffs, natural_cubic_spline_coeffs)
from .losses import MaskedTemporalLoss, RMSELoss, TemporalLossWrapper, masked_mean  # noqa: F401
