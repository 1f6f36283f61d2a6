// Kernel instantiations for the 100-job node bucket (one TU per bucket so the
// instantiations compile in parallel).
#include "pfsp_engine.hpp"

namespace tts {
TTS_PFSP_DEFINE_BUCKET(100)
// 51-100 jobs on front nodes with 128-bit job sets (TTS_FRONT_WIDE=1)
TTS_PFSP_DEFINE_FRONT_BUCKET(100)
}  // namespace tts
