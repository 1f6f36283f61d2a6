// Kernel instantiations for the 50-job node bucket (one TU per bucket so the
// instantiations compile in parallel).
#include "pfsp_engine.hpp"

namespace tts {
TTS_PFSP_DEFINE_BUCKET(50)
// 21-50 jobs on front nodes with 64-bit job sets
TTS_PFSP_DEFINE_FRONT_BUCKET(50)
}  // namespace tts
