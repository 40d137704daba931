"""ctypes binding of the C ABI in include/firefly/ff_api.h (libfirefly_hip.so, built in-tree by
``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C gpupathtracer_amd/csrc``).

There is no CPU fallback: if the HIP library is missing, importing this module's ``load()`` raises.

This module is the façade every caller goes through (``from gpupathtracer_amd import lib``); the code is in three modules by concern:

  _abi    where the library is, ``load()``, the prototype table (``PROTOTYPES``, ``EXPORTS``), ``check`` / ``FireflyError``
  host    everything that needs no GPU: file I/O, host tables and samplers, the ``*_params`` builders, the ``*_host`` filter twins
  tracer  ``Tracer``, ``MultiTracer`` and the ``dist_*`` helpers: what needs ``ff_create``
"""
import ctypes as C  # noqa: F401  (lib.C, lib.T and lib.np are part of the surface: callers spell lib.C.byref, lib.T.FF_OK)

import numpy as np  # noqa: F401

from . import types as T  # noqa: F401
from ._abi import EXPORTS, LIB_PATH, PROTOTYPES, FireflyError, check, load  # noqa: F401
from .host import *  # noqa: F401,F403
from .tracer import *  # noqa: F401,F403
