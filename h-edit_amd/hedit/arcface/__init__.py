from .arcface_model import IDLoss, Backbone  # noqa: F401
from .face_parsing import FaceParsing, face_mask  # noqa: F401
