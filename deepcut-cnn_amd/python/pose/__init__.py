from .people import MIRROR_MPII14, estimate_people, track_people, people_boxes  # noqa: F401
