from .meshes import Meshes  # noqa: F401
from .pointclouds import Pointclouds  # noqa: F401
from .rgbdimages import RGBDImages  # noqa: F401
from .tsdfvolume import TSDFVolume  # noqa: F401
from .utils import pointclouds_from_rgbdimages, rgbdimages_from_pointclouds  # noqa: F401
