"""MI355X-native replacement of the reference's frame-wise DNN trainer hot path
(`BP_GPU` in yongxuUSTC/DNN-for-speech-enhancement).  The product is the gfx950 HIP library
`libbp_hip.so` behind the C ABI in include/bp_c_api.h; this package is its Python host mirror.
(The directory name contains '-', import it through `dnnse_amd.py` at the repo root.)"""
from ._abi import *        # noqa: F401,F403  (each public name is listed once, in its module's __all__)
from .bp_gpu import *      # noqa: F401,F403
from .signal import *      # noqa: F401,F403
from .rbm import *         # noqa: F401,F403
from .weights_init import glorot_net  # noqa: F401
