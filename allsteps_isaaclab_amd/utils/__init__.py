"""Counterparts of the ``isaaclab.utils`` sub-modules the env cfgs use."""
