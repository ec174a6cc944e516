from . import fusionutils  # noqa: F401
from .icpslam import ICPSLAM  # noqa: F401
from .kinectfusion import KinectFusion  # noqa: F401
from .pointfusion import PointFusion  # noqa: F401
