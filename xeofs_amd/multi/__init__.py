from .cca import CCA  # noqa: F401
