from .people import estimate_people, people_boxes  # noqa: F401
