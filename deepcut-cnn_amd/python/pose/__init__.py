from .people import MIRROR_MPII14, SKELETON_MPII14, estimate_people, track_people, draw_people, draw_heatmap, people_boxes  # noqa: F401
