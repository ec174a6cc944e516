"""Odometry provider interface (reference odometry/base.py:6-19) -- the plugin seam of the path.

The contract ICPSLAM relies on (slam/icpslam.py:243):
``provide(maps_pointclouds: Pointclouds, frames_pointclouds: Pointclouds) -> torch.Tensor (B, 1, 4, 4)``,
the rigid transform that aligns every frame cloud to its map cloud."""
import abc

__all__ = ["OdometryProvider"]


class OdometryProvider(abc.ABC):
    def __init__(self, *params):
        """Providers keep their own parameters; the base class has no state."""

    @abc.abstractmethod
    def provide(self, *args, **kwargs):
        """One odometry estimate per batch element; concrete providers define the arguments."""
        raise NotImplementedError


def check_levels_numiters(name, numiters, levels):
    """The (numiters, levels) of the coarse-to-fine provider called `name` -> numiters as `levels` counts (an int: at every level)."""
    if not isinstance(levels, int) or isinstance(levels, bool) or levels < 1:
        raise ValueError("{}: levels should be a positive integer. Got {!r}.".format(name, levels))
    if isinstance(numiters, int) and not isinstance(numiters, bool):
        numiters = (numiters,) * levels
    numiters = tuple(numiters)
    if len(numiters) != levels or any(not isinstance(n, int) or isinstance(n, bool) or n < 0 for n in numiters):
        raise ValueError("{}: numiters should be an integer or {} non-negative integers (finest level first). "
                         "Got {!r}.".format(name, levels, numiters))
    return numiters


def check_init(init, B):
    """`init` of a provide(): None, or B transforms shaped (..., 4, 4)."""
    if init is not None and (init.numel() != 16 * B or tuple(init.shape[-2:]) != (4, 4)):
        raise ValueError("Expected init to have shape ({0}, 1, 4, 4). Got {1}.".format(B, tuple(init.shape)))
