"""Stand-in package: see color.py."""
