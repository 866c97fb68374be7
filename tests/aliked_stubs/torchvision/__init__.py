"""Test-only stand-in (see ../README.md): just what the reference's ALIKED module imports."""
from . import models, ops  # noqa: F401
