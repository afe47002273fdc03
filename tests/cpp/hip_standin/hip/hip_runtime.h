// A host stand-in for the part of the HIP runtime that csrc/pipeline.cpp, multi.cpp, hostmem.cpp
// and knobs.cpp use, written from HIP's documented behaviour (tests/cpp/hip_standin/standin.cpp
// implements it on CPU threads).  It declares those 26 calls and nothing else; the numeric values
// of the enumerators are this file's own and mean nothing outside it.
#pragma once
#include <cstddef>
#include <cstdint>

extern "C" {

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue,
    hipErrorOutOfMemory,
    hipErrorInvalidDevice,
    hipErrorInvalidResourceHandle,
    hipErrorNotReady,
    hipErrorNotSupported
} hipError_t;

typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef void* hipDeviceptr_t;

typedef enum hipMemcpyKind {
    hipMemcpyHostToHost,
    hipMemcpyHostToDevice,
    hipMemcpyDeviceToHost,
    hipMemcpyDeviceToDevice,
    hipMemcpyDefault
} hipMemcpyKind;

typedef enum hipMemoryType {
    hipMemoryTypeUnregistered,
    hipMemoryTypeHost,
    hipMemoryTypeDevice
} hipMemoryType;

typedef struct hipPointerAttribute_t {
    hipMemoryType type;
    int device;
    void* devicePointer;
    void* hostPointer;
} hipPointerAttribute_t;

typedef enum hipPointer_attribute {
    HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR,
    HIP_POINTER_ATTRIBUTE_RANGE_SIZE
} hipPointer_attribute;

enum : unsigned {
    hipStreamDefault = 0u,
    hipStreamNonBlocking = 1u,
    hipEventDefault = 0u,
    hipEventDisableTiming = 2u,
    hipHostMallocDefault = 0u,
    hipHostMallocPortable = 1u,
    hipHostMallocNumaUser = 0x20000000u
};

hipError_t hipMalloc(void** ptr, size_t bytes);
hipError_t hipFree(void* ptr);
hipError_t hipHostMalloc(void** ptr, size_t bytes, unsigned flags);
hipError_t hipHostFree(void* ptr);
hipError_t hipMemset(void* dst, int value, size_t bytes);
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                          hipStream_t stream);
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                            size_t height, hipMemcpyKind kind, hipStream_t stream);

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned flags);
hipError_t hipStreamCreateWithPriority(hipStream_t* stream, unsigned flags, int priority);
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest);
hipError_t hipStreamDestroy(hipStream_t stream);
hipError_t hipStreamSynchronize(hipStream_t stream);
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags);

hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t event);
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream);
hipError_t hipEventSynchronize(hipEvent_t event);
hipError_t hipEventQuery(hipEvent_t event);

hipError_t hipGetDevice(int* device);
hipError_t hipSetDevice(int device);
hipError_t hipGetDeviceCount(int* count);
hipError_t hipGetLastError(void);
const char* hipGetErrorString(hipError_t e);

hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attr, const void* ptr);
hipError_t hipPointerGetAttribute(void* data, hipPointer_attribute attr, hipDeviceptr_t ptr);
hipError_t hipDeviceGetPCIBusId(char* bus_id, int len, int device);

}  // extern "C"
