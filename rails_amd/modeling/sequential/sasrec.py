"""Import-path mirror of the reference's modeling/sequential/sasrec.py: `from rails_amd.modeling.sequential.sasrec import SASRec`."""
from ...sasrec import SASRec  # noqa: F401
