"""Application modules of AMPIS on the native path (ampis/applications): powder characterisation."""
from . import powder
