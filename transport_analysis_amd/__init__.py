"""transport_analysis_amd — MI355X-native time-correlation kernels behind the
transport-analysis API (VelocityAutocorr, ViscosityHelfand), MDAnalysis' EinsteinMSD, ConductivityHelfand and its species-resolved form, OnsagerHelfand, and their Green-Kubo
(velocity) twins, ConductivityGreenKubo and OnsagerGreenKubo, and the intermediate scattering functions F_s(k, t) and F(k, t),
IntermediateScattering, with their species-resolved partials F_ab(k, t) and S_ab(k), PartialScattering, and their real-space partners, the self van Hove function G_s(r, t) with the non-Gaussian parameter,
VanHoveSelf, and the distinct van Hove function G_d(r, t) with the radial distribution function g(r), VanHoveDistinct, and
the longitudinal and transverse current correlation functions C_L(k, t) and C_T(k, t), CurrentCorrelation, and the
self-overlap Q(t) with the four-point susceptibility chi_4(t), DynamicSusceptibility, and the four-point structure factor
S_4(k, t) of the overlap field, FourPointStructureFactor, and the rotational correlation functions
C_1(t), C_2(t) of molecule-fixed unit vectors with their dipole sum, OrientationalCorrelation, and the intermittent and
continuous pair population correlation functions with the lifetimes of ion pairs and solvation contacts, PairLifetime, and
of hydrogen bonds with a donor-hydrogen-acceptor angle criterion, HydrogenBondLifetime, and the residence times of atoms in
the solvation shell of a whole group, ShellResidence, with the mean squared displacement of the atoms while they stay in that
shell, ShellMSD, and the reorientation of their molecules while they stay there, ShellOrientation, and the autocorrelations
of the Rouse normal modes and of the end-to-end vector of chains, RouseModes."""
__version__ = "0.1.0"

from .velocityautocorr import VelocityAutocorr  # noqa: F401
from .viscosity import ViscosityHelfand  # noqa: F401
from .msd import EinsteinMSD  # noqa: F401
from .conductivity import ConductivityHelfand  # noqa: F401
from .onsager import OnsagerHelfand  # noqa: F401
from .greenkubo import ConductivityGreenKubo, OnsagerGreenKubo  # noqa: F401
from .scattering import IntermediateScattering, kvectors_from_box  # noqa: F401
from .partial_scattering import PartialScattering  # noqa: F401
from .current_correlation import CurrentCorrelation  # noqa: F401
from .vanhove import VanHoveSelf, log_lags  # noqa: F401
from .vanhove_distinct import VanHoveDistinct  # noqa: F401
from .susceptibility import DynamicSusceptibility  # noqa: F401
from .four_point import FourPointStructureFactor  # noqa: F401
from .orientation import OrientationalCorrelation, group_indices  # noqa: F401
from .pair_lifetime import PairLifetime  # noqa: F401
from .hbond_lifetime import HydrogenBondLifetime  # noqa: F401
from .shell_residence import ShellResidence  # noqa: F401
from .shell_msd import ShellMSD  # noqa: F401
from .shell_orientation import ShellOrientation  # noqa: F401
from .rouse import RouseModes  # noqa: F401
