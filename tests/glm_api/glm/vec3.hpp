// glm/vec3.hpp of the stand-in (glm.hpp holds the whole interface)
#include "glm.hpp"
