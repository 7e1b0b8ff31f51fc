"""waterlily_amd -- MI355X-native backend for WaterLily's `sim_step!` hot path."""
from .body import AutoBody, NoBody, measure, norm2  # noqa: F401
from . import budget  # noqa: F401
from .budget import Budget  # noqa: F401
from .downsample import Downsampler, DownsampleWriter  # noqa: F401
from . import forces  # noqa: F401
from .forces import Forces  # noqa: F401
from . import hist  # noqa: F401
from .hist import Axis, Histogram  # noqa: F401
from .mesh import MeshBody  # noqa: F401
from .probes import Probes, Tracers, interp  # noqa: F401
from . import regions  # noqa: F401
from .regions import Regions, RegionSeries  # noqa: F401
from .render import Renderer  # noqa: F401
from . import scene  # noqa: F401
from .scene import Camera, Scene  # noqa: F401
from . import twopoint  # noqa: F401
from .twopoint import TwoPoint, Value  # noqa: F401
from . import volume  # noqa: F401
