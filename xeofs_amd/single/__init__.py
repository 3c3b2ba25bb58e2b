from .archetypal import ArchetypalAnalysis  # noqa: F401
from .dineof import DINEOF  # noqa: F401
from .eeof import ExtendedEOF  # noqa: F401
from .eof import EOF, ComplexEOF, HilbertEOF  # noqa: F401
from .eot import EOT  # noqa: F401
from .gwpca import GWPCA  # noqa: F401
from .ica import ICA  # noqa: F401
from .kmeans import KMeans  # noqa: F401
from .lfca import LFCA  # noqa: F401
from .opa import OPA  # noqa: F401
from .pop import POP  # noqa: F401
from .sparse_pca import SparsePCA  # noqa: F401
from .spectral_eof import SpectralEOF  # noqa: F401
from .teleconnectivity import Teleconnectivity  # noqa: F401
from .trend_eof import TrendEOF  # noqa: F401
from .eof_rotator import ComplexEOFRotator, EOFRotator, HilbertEOFRotator  # noqa: F401
