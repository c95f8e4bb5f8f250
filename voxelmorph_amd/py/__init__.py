"""`voxelmorph.py` of the reference: backend-independent utilities (voxelmorph/py/__init__.py)."""
from . import utils  # noqa: F401
