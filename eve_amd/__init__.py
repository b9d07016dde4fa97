"""eve_amd: MI355X-native (gfx950) implementation of the EVE hot path -- the EyeNet encoder and the
RefineNet point-of-gaze refiner of swook/EVE -- as torch.nn.Module drop-ins over hand-written HIP
kernels (libeve_hip.so, C ABI in include/eve_hip.h)."""
from .config import HotPathConfig, get_config, reset_standalone_config  # noqa: F401
from .eye_net import EyeNet  # noqa: F401

__all__ = ['EyeNet', 'RefineNet', 'EVE', 'EVEStream', 'OverlaySpec', 'GazeEventSpec', 'SaccadeSpec', 'PursuitSpec', 'GazeHistorySpec', 'AoiSpec', 'PupilSpec', 'ScreenLuminanceSpec', 'EyeGateSpec', 'BlinkSpec', 'SurfaceLayout', 'screen_calibration_samples', 'fit_screen_map', 'evaluate_screen_map', 'apply_screen_map', 'get_config', 'HotPathConfig', 'reset_standalone_config']


def __getattr__(name):
    if name == 'RefineNet':
        from .refine_net import RefineNet
        return RefineNet
    if name == 'EVE':
        from .eve import EVE
        return EVE
    if name == 'EVEStream':
        from .stream import EVEStream
        return EVEStream
    if name == 'OverlaySpec':
        from .data import OverlaySpec
        return OverlaySpec
    if name == 'GazeEventSpec':
        from .data import GazeEventSpec
        return GazeEventSpec
    if name == 'SaccadeSpec':
        from .data import SaccadeSpec
        return SaccadeSpec
    if name == 'PursuitSpec':
        from .data import PursuitSpec
        return PursuitSpec
    if name == 'GazeHistorySpec':
        from .data import GazeHistorySpec
        return GazeHistorySpec
    if name == 'AoiSpec':
        from .data import AoiSpec
        return AoiSpec
    if name == 'PupilSpec':
        from .data import PupilSpec
        return PupilSpec
    if name == 'ScreenLuminanceSpec':
        from .data import ScreenLuminanceSpec
        return ScreenLuminanceSpec
    if name == 'EyeGateSpec':
        from .data import EyeGateSpec
        return EyeGateSpec
    if name == 'BlinkSpec':
        from .data import BlinkSpec
        return BlinkSpec
    if name == 'SurfaceLayout':
        from .data import SurfaceLayout
        return SurfaceLayout
    if name in ('screen_calibration_samples', 'fit_screen_map', 'evaluate_screen_map', 'apply_screen_map'):
        from . import data
        return getattr(data, name)
    raise AttributeError(name)
