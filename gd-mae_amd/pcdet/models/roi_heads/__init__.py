from .roi_head_template import RoIHeadTemplate
from .graphrcnn_head import GraphRCNNHead

__all__ = {
    'RoIHeadTemplate': RoIHeadTemplate,
    'GraphRCNNHead': GraphRCNNHead,
}
